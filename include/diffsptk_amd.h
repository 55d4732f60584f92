/*
 * diffsptk_amd -- C-ABI of the MI355X (gfx950) device backend for the STFT -> mel-cepstrum
 * and LPC analysis hot path of sp-nitech/diffsptk (v4.0.0).
 *
 * The reference is a pure-Python library over PyTorch: it has NO FFI/plugin interface.  Its
 * operator boundary is the static `_forward(x, **precomputed)` method of every module
 * (diffsptk/modules/base.py:38-101).  Each entry point below is what a binding for one such
 * `_forward` (and its autograd-derived backward, SURVEY.md section 3.5) binds; the reference
 * symbol it replaces is cited per function.  INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (HIP, same process / same HIP runtime as the caller)
 *    unless the name ends in `_host`; the caller (PyTorch) allocates all buffers;
 *  - tensors are dense row-major ("contiguous"); leading batch dims are flattened by the caller;
 *  - ALIGNMENT: a tensor pointer needs the natural alignment of its element and nothing more (4 bytes for DSA_F32, 8 for
 *    DSA_F64 and for the float pairs of a complex64 tensor): a contiguous view that starts anywhere inside an allocation is a
 *    valid argument, input or output.  The library chooses wider (8- / 16-byte) accesses itself, per call or per run inside a
 *    kernel, where the address it is handed allows them, and computes the same values where it does not
 *    (tests/test_gpu_alignment.py);
 *  - a ZERO count (B, F, n = 0: an empty batch, which the reference's ATen ops accept) is a successful no-op: the sizes are
 *    validated, the pointers are not looked at (an empty tensor has no storage; its data pointer is NULL);
 *  - `dtype`: DSA_F32 or DSA_F64 (the reference supports both; CI runs float64);
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls are asynchronous
 *    on that stream, re-entrant, and keep no mutable global state: the library keeps NO device memory (the only
 *    allocations it makes are transient, stream-ordered hipMallocAsync / hipFreeAsync pairs inside one call: the partial
 *    spans of dsa_stft_bwd / dsa_istft_fwd for frame geometries other than L = 400, P = 80 / 160 -- those run the
 *    one-launch kernel that needs none -- and the zero waveform of the generic inverse path).
 *    The tuned kernels need two kinds of workspace, both owned by the caller:
 *      `scratch`  DSA_SCRATCH_BYTES of device memory per call (work-queue counters of the persistent kernels),
 *                 zeroed by the library on `stream`; it must not be shared by calls that can overlap in time (one
 *                 buffer per stream, or one fresh buffer per call from a stream-ordered allocator).  scratch = NULL
 *                 selects the kernel family that needs none (DSA_ALGO_TUNED then fails with
 *                 DSA_ERR_INVALID_ARGUMENT);
 *      `images`   per-CONFIGURATION constants prepared once (dsa_mcep_prepare), read-only afterwards and
 *                 shareable by any number of concurrent calls on the same device;
 *    the only per-process state is, per kernel, the set of devices whose dynamic-LDS limit has been raised;
 *  - return value: DSA_OK (0) or a negative dsa_status; dsa_last_error() gives the message of
 *    the last failure on the calling thread.  Nothing throws across the boundary.
 *  - argument VALIDATION of user-facing options (ValueError text etc.) is done by the host
 *    layer exactly like the reference's `_check`; the library re-checks only what would make a
 *    launch unsafe.
 */
#ifndef DIFFSPTK_AMD_H
#define DIFFSPTK_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSA_VERSION 148 /* 0.4.2: dsa_pitch_spec_vjp_gather with T = 1 sums every column of the one frame (the replicate padding clamps them all to the one sample; 147 dropped the columns behind the middle); 0.4.1: + dsa_pitch_spec / dsa_pitch_spec_vjp_frames / dsa_pitch_spec_vjp_gather (the pitch-adaptive spectral envelope of CheapTrick: a frame from the waveform to the formatted envelope in one workgroup and one launch, float64 inside, and the adjoint down to the waveform in two launches without atomics); 0.4.0: + dsa_ap_qmf / dsa_ap_qmf_vjp / dsa_ap_tandem / dsa_ap_tandem_vjp (band aperiodicity by TANDEM-STRAIGHT: a level of the QMF pyramid and its transpose, the per-band least-squares fits of a frame with their own regulariser escalation and the interpolated, clipped output in one launch, and the adjoint down to the band signals without atomics); 0.3.9: + dsa_world_synth_pulses / dsa_world_synth_responses / dsa_world_synth_overlap_add / dsa_world_synth_vjp_pulses / dsa_world_synth_vjp_frames (WORLD synthesis: the time base and pulse list of an utterance in one workgroup, a pulse's periodic and aperiodic response through four complex transforms in LDS, the overlap-add as a gather, and the adjoint down to sp and ap in two launches); 0.3.8: + DSA_ALGO_FULL_CHAINS (the tuned mel-cepstral forward runs the first clamp(n_iter - 6, 0, 2) Newton steps on one-term binary16 chains; the flag keeps every step on three terms); 0.3.7: + dsa_vq_search / dsa_vq_accum / dsa_vq_update / dsa_vq_lookup / dsa_vq_vjp (vector quantisation and the Linde-Buzo-Gray codebook design: nearest-codeword search on float64 sums, per-codeword counts and float64 sums in fixed-order segments without atomics, centroids with the iteration's three scalars, the lookup and the quantiser's adjoint); 0.3.6: + dsa_yingram / dsa_yingram_vjp / dsa_frame_yingram (Yingram: YIN's cumulative-mean-normalised difference function on a semitone grid, from frames or from the waveform in one launch, and its adjoint; lag sums directly or through the LDS transform); 0.3.5: + dsa_gmm_prepare / dsa_gmm_estep / dsa_gmm_accum / dsa_gmm_update / dsa_gmm_regress / dsa_gmm_transform (Gaussian mixture models: one EM iteration as factorisation, E-step, weighted moment sums and M-step on the device, and the conversion of a joint-density model); 0.3.4: + dsa_dtw / dsa_dtw_vjp / dsa_dtw_path (dynamic time warping with a soft minimum: the aligned distance of two vector sequences by an anti-diagonal wavefront, its gradient by the reverse sweep, the Viterbi path from the saved tables); 0.3.3: + DSA_ALGO_FIXED_STEPS (the tuned mel-cepstral forward stops a frame's Newton iteration once its update is rounding noise; the flag runs every step); 0.3.2: + dsa_delta / dsa_delta_vjp, dsa_mlpg, dsa_mcpf / dsa_mcpf_vjp (parameter generation: delta features, maximum likelihood parameter generation by a banded Cholesky solve, mel-cepstrum postfiltering in closed form); 0.3.1: + dsa_mdct_analysis / dsa_mdct_synthesis (MDCT / MDST and their inverses: window, fold, DCT-IV through a quarter-length complex FFT and overlap-add in one launch each way; each is the other's adjoint); 0.3.0: + dsa_excite (pitch to excitation: the voiced shapes of ExcitationGeneration on a segmented float64 phase sum, one launch); 0.2.9: + dsa_mlsacheck / dsa_mlsacheck_vjp (the stability check of the MLSA filter: the mel-cepstrum scaled or clipped where the amplitude of its gain-free part passes the threshold of the Pade approximation, forward and adjoint); 0.2.8: + dsa_lpc2lsp_fwd / _bwd, dsa_lsp2lpc_fwd / _bwd, dsa_lspcheck_fwd / _bwd (line spectral pairs by a Chebyshev-series root search, back by a product of real sections, and their stability check, forward and adjoint); 0.2.7: + dsa_lpc2par_fwd / _bwd, dsa_par2lpc_fwd / _bwd, dsa_lpccheck_fwd / _bwd (the step-down and step-up recursions between LPC and PARCOR coefficients and the stability check built from them, forward and adjoint); 0.2.6: + dsa_pqmf_fwd / _bwd, dsa_ipqmf_fwd / _bwd (pseudo-QMF analysis and synthesis with decimation / interpolation folded in), dsa_interpolate_fwd / _bwd; 0.2.5: + dsa_plp_fwd / dsa_plp_bwd (PLP after the filter bank, forward and adjoint); 0.2.4: + dsa_poledf_fwd / dsa_poledf_bwd (the time-variant all-pole filter, forward and adjoint); 0.2.3: + DSA_ALGO_RESERVE_CUS; a zero count is a no-op before any pointer check; 0.2.2: + dsa_mcep_newton_glogx_h (glogx of the 48 kHz analysis in one pass after the sweep; dsa_mcep_newton_resid_h_bwd takes glogx = NULL); twin workgroups in dsa_mcep_newton_steps; 0.2.1: + dsa_mcep_resid_bwd_images_bytes / _prepare, dsa_mcep_newton_resid_h_bwd (the 48 kHz analysis with a gradient: the step's backward in two launches); wide tiles in dsa_mcep_newton_steps; 0.2.0: + dsa_mcep_newton_steps, dsa_stft_mcep_opts_fwd, DSA_ALGO_OVERLAPPED_LAUNCHES, DSA_ALGO_PAD_MODE, packed STFT kernels for fft_length 1024 / 2048 and for every pad mode at 512; 0.1.9: + dsa_mgcep_step_solve, dsa_mgcep_step_bwd_h, dsa_mcep_resid_images_bytes / _prepare, dsa_mcep_newton_resid_h; 0.1.8: + dsa_frame_window_lpc_bwd, DSA_LPC_EXACT_LAGSUMS, DSA_ALGO_HIST_HAS_RT; 0.1.7: + dsa_gnorm_fwd, dsa_mgcep_gain, DSA_LPC_SCRATCH_IS_CLEAN; 0.1.6: + dsa_mcep_newton_update_bwd; 0.1.5: + dsa_mcep_newton_resid; 0.1.4: dsa_stft_mcep_fwd (STFT -> mel-cepstrum in one launch), dsa_rows_gemm, dsa_rows_ew, dsa_mcep_newton_update */

typedef enum {
    DSA_OK = 0,
    DSA_ERR_INVALID_ARGUMENT = -1,
    DSA_ERR_UNSUPPORTED = -2,
    DSA_ERR_LAUNCH = -3,
    DSA_ERR_NO_DEVICE = -4
} dsa_status;

enum { DSA_F32 = 0, DSA_F64 = 1 };
/* size of the per-call `scratch` the tuned persistent kernels draw their work items through */
#define DSA_SCRATCH_BYTES 64
/* F.pad modes of Frame (frame.py:134-137) */
enum { DSA_PAD_CONSTANT = 0, DSA_PAD_REFLECT = 1, DSA_PAD_REPLICATE = 2, DSA_PAD_CIRCULAR = 3 };
/* fftr.py:110-121 */
enum { DSA_FFTR_COMPLEX = 0, DSA_FFTR_REAL = 1, DSA_FFTR_IMAG = 2, DSA_FFTR_AMPLITUDE = 3, DSA_FFTR_POWER = 4 };
/* spec.py:123-132 (+ complex pass-through of stft.py:211-222) */
enum { DSA_SPEC_DB = 0, DSA_SPEC_LOGMAG = 1, DSA_SPEC_MAG = 2, DSA_SPEC_POWER = 3, DSA_SPEC_COMPLEX = 4,
       /* the inverse real transform's weights c_k / nfft (c = 1 at k = 0 and nfft/2, else 2) folded into the STFT
        * kernels: in dsa_stft_bwd / dsa_istft_fwd the complex spectrogram to INVERT (istft.py:186-193) is weighted
        * while it is loaded; in dsa_stft_fwd the complex output is weighted (the adjoint: the backward of the ISTFT) */
       DSA_SPEC_COMPLEX_INV = 5 };
/* acorr.py:94-107 */
enum { DSA_ACORR_NAIVE = 0, DSA_ACORR_NORMALIZED = 1, DSA_ACORR_BIASED = 2, DSA_ACORR_UNBIASED = 3 };
/* kernel selection: AUTO picks the tuned gfx950 kernel when the configuration allows it */
enum { DSA_ALGO_AUTO = 0, DSA_ALGO_GENERIC = 1, DSA_ALGO_TUNED = 2 };
/* OR-ed into `algo` of dsa_mcep_fwd: the caller guarantees that `scratch` is ZERO on entry (zeroed once, at allocation) and is used
 * by one call at a time; the library then skips its per-call reset (a 5 us fill launch and a kernel boundary per call) -- the
 * persistent kernel leaves the counters zeroed when its last wave retires, with or without this flag. */
#define DSA_ALGO_SCRATCH_IS_CLEAN 0x100
/* OR-ed into `algo` of dsa_mcep_bwd: `scratch` is DSA_MCEP_BWD_WORKSPACE_BYTES long (the counters + a hand-over area).  The tuned
 * backward then cuts a short last round of tiles into pieces of Newton steps that pass their state through it, so that every wave
 * slot ends the launch busy (3 200 tiles on 1 024 slots: 3.3 rounds instead of 4).  Without the flag: DSA_SCRATCH_BYTES, no split. */
#define DSA_ALGO_SCRATCH_HAS_WORKSPACE 0x200
#define DSA_MCEP_BWD_WORKSPACE_BYTES (DSA_SCRATCH_BYTES + 512 * 16 * 32 * 4)
/* OR-ed into `algo` of dsa_mcep_fwd / dsa_stft_mcep_fwd / dsa_mcep_bwd (0.1.8): `mc_hist` continues behind the (n_iter + 1, F, M + 1)
 * iterates with (n_iter, F, 2 M + 1) float32 rows -- every Newton step's rt = e E (mcep.py:212-215).  The tuned forward writes them, the
 * tuned backward reads them instead of recomputing its second forward chain -- and runs as the two-waves-per-SIMD kernel
 * (csrc/mcep_mfma_bwd2_f16.h: 1.56 -> 1.1-1.2 ms per 204 800 frames for 196 more bytes per frame and step).  Both calls of a pair must agree on the flag; the generic kernels ignore the extra room. */
#define DSA_ALGO_HIST_HAS_RT 0x400
/* OR-ed into `algo` of dsa_mcep_fwd / dsa_stft_mcep_fwd (0.2.0): the caller alternates consecutive, independent launches between TWO
 * streams (each with its own `scratch`).  A launch whose tiles do not fill a whole number of rounds of the chip's 2 048 wave slots
 * (204 800 frames = 12 800 tiles = 6.25 rounds) ends in a short round.  Without the flag that round runs one wave per SIMD on every
 * CU (the fastest way to finish ONE launch: 0.8 of a full round's time, the rest of the chip idle).  With it the short round is
 * packed onto the first ceil(rest / 8) workgroups at two waves per SIMD and every other workgroup EXITS when the shared tiles run
 * out, so that the next launch's workgroups -- waiting on the other stream for LDS -- start on the freed CUs (measured: 0.5945 ->
 * 0.5685 ms per 204 800 frames over 200 steps; the ideal is 6.25 rounds per launch instead of 6.8).  Same tiles, same arithmetic,
 * same results bit for bit; a lone launch gets 0.2 of a round slower. */
#define DSA_ALGO_OVERLAPPED_LAUNCHES 0x800
/* OR-ed into `algo` of dsa_stft_mcep_fwd (0.2.0): the padding mode of Frame (frame.py:130-137; DSA_PAD_*, 0 = constant) for the
 * samples a frame reads outside its utterance -- the one-launch step then covers ShortTimeFourierTransform(mode=...) too. */
#define DSA_ALGO_PAD_MODE(m) (((m) & 3) << 12)
/* OR-ed into `algo` of dsa_mcep_fwd / dsa_stft_mcep_fwd / dsa_stft_mcep_opts_fwd (0.2.3): the persistent launch leaves n (<= 63) of the
 * 256 CUs free.  A persistent workgroup fills its CU's LDS and registers, so a kernel of ANOTHER stream that has to run beside the
 * launch -- RCCL's all-gather of the previous batch's features (SURVEY 8(e)) -- could otherwise only start in the launch's tail and the
 * next launch would queue behind it: the exchange would be serial with the analysis instead of hidden behind it.  Same tiles, same
 * arithmetic, same bits.  The launcher leaves at least n and up to 2 n CUs where that costs no further round of tiles.  Measured with a stand-in
 * collective (profiles/r06_reserve_cus_ab.txt): what matters most is WHEN the caller waits for the collective -- two batches later, 8 CUs
 * suffice (0.618 ms per step against 0.584 alone); one batch later the two run in series whatever is reserved below 16.  dist.py sets it. */
#define DSA_ALGO_RESERVE_CUS(n) (((n) & 63) << 16)
#define DSA_ALGO_RESERVED_CUS(algo) (((algo) >> 16) & 63)
/* OR-ed into `algo` of dsa_mcep_fwd / dsa_stft_mcep_fwd / dsa_stft_mcep_opts_fwd (0.3.3): run every one of the n_iter Newton steps.
 * Without the flag the tuned forward (float32, fft_length 512, cep_order 24) treats n_iter as the LARGEST number of steps: a frame's
 * iteration ends with the first step k whose update x satisfies, with u_k = |x|_inf / max(1, |mc|_inf) -- mc the iterate the step started
 * from --, either u_k <= 2^-20, or u_k <= 2^-16 and u_k <= u_(k-1) / 16: Newton's quadratic phase, in which the NEXT update would
 * be below 2^-20; never at step 1.  That update is still applied, every later one of the frame is discarded: from there on float32
 * Newton steps only add the solve's rounding error to a finished answer (DESIGN.md 3.1).  The rule reads the frame's own values only, so a frame's result does
 * not depend on its batch, its neighbours or the kernel path; a frame with a NaN never stops early.  Without a history (mc_hist = NULL)
 * a 16-frame tile leaves the step loop once all its frames have stopped; with one, all n_iter steps run with the stopped frames'
 * updates masked, so the iterates repeat from the stopping step on and the rt rows are complete.  With the flag and DSA_ALGO_FULL_CHAINS the results
 * are those of 0.3.2 bit for bit.  The generic kernels, dsa_mgcep_* and the 48 kHz family always run exactly n_iter steps. */
#define DSA_ALGO_FIXED_STEPS 0x4000
/* OR-ed into `algo` of dsa_mcep_fwd / dsa_stft_mcep_fwd / dsa_stft_mcep_opts_fwd (0.3.8): every Newton step on three-term chains.
 * Each matrix chain of a step of the tuned forward is three binary16 products, ah bh + ah bl + al bh, for float32-grade accuracy.
 * Without the flag step k (1-based) is COARSE when k <= clamp(n_iter - 6, 0, 2): its two chains run the ah bh product alone (operands
 * good to 2^-11).  Newton's method corrects itself: those steps move the iterate by 5e-2 .. 2e-1 of its size, and at least six full
 * steps follow every coarse one (n_iter <= 6 has none).  The schedule depends on k and n_iter only, with or without
 * DSA_ALGO_FIXED_STEPS, so a frame's result still depends on nothing but its own values.  No frame stops on a coarse step (all-zero and
 * padding-like frames, which stopped after step 1 - 2, now run to about step 4 - 5).  With the flag, or DSA_MCEP_FULL_CHAINS=1 in the
 * environment, the results are those of 0.3.7 bit for bit; with DSA_ALGO_FIXED_STEPS as well, those of 0.3.2. */
#define DSA_ALGO_FULL_CHAINS 0x8000

int dsa_version(void);
const char* dsa_last_error(void);
/* number of visible HIP devices, or a negative dsa_status */
int dsa_device_count(void);
/* name of the kernel family the last call on this thread dispatched to (for tests/profiles) */
const char* dsa_last_kernel(void);

/* N = (T-1)/P + 1 frames for T >= 1 (frame.py:130-138: padded length is T + L - 1). */
int64_t dsa_num_frames(int64_t T, int32_t P);

/* ------------------------------------------------------------------ a1  Frame
 * Frame._forward, diffsptk/modules/frame.py:120-141.
 * x:(B,T) -> y:(B,N,L); bit-exact gather copy (zmean subtracts the frame mean). */
int dsa_frame_fwd(const void* x, int64_t B, int64_t T, int32_t L, int32_t P, int32_t center,
                  int32_t zmean, int32_t pad_mode, int32_t dtype, void* y, void* stream);
/* gy:(B,N,L) -> gx:(B,T): deterministic overlap-add (adjoint of pad + unfold + zmean). */
int dsa_frame_bwd(const void* gy, int64_t B, int64_t T, int32_t L, int32_t P, int32_t center,
                  int32_t zmean, int32_t pad_mode, int32_t dtype, void* gx, void* stream);

/* ------------------------------------------------------------------ a2  Window
 * Window._forward, window.py:185-193.  x:(F,L) * w:(L) -> y:(F,L2), zero padded (L2>=L) or
 * cropped (L2<L, F.pad with a negative amount). */
int dsa_window_fwd(const void* x, int64_t F, int32_t L, const void* w, int32_t L2, int32_t dtype,
                   void* y, void* stream);
/* gy:(F,L2) -> gx:(F,L) and, if gw != NULL, gw:(L) += sum_f gy*x (learnable window). */
int dsa_window_bwd(const void* gy, const void* x, int64_t F, int32_t L, const void* w, int32_t L2,
                   int32_t dtype, void* gx, void* gw, void* stream);

/* ------------------------------------------------------------------ a3  fftr
 * RealValuedFastFourierTransform._forward, fftr.py:136-151 (torch.fft.rfft + formatter).
 * x:(F,len_in) zero-padded/cropped to nfft -> y:(F,nfft/2+1) real, or interleaved (re,im)
 * pairs for DSA_FFTR_COMPLEX.  twiddle:(nfft,2) = (cos, -sin)(2 pi m / nfft), device. */
int dsa_fftr_fwd(const void* x, int64_t F, int32_t len_in, int32_t nfft, int32_t out_format,
                 const void* twiddle, int32_t dtype, void* y, void* stream);
int dsa_fftr_bwd(const void* gy, const void* x, int64_t F, int32_t len_in, int32_t nfft,
                 int32_t out_format, const void* twiddle, int32_t dtype, void* gx, void* stream);

/* ------------------------------------------------------------------ a4  Spectrum
 * Spectrum._forward, spec.py:152-178.  b:(F,lb) and/or a:(F,la) (either may be NULL, not both).
 * y:(F,nfft/2+1) = format(max(|K B/A|^2 + eps, floor)). */
int dsa_spec_fwd(const void* b, int32_t lb, const void* a, int32_t la, int64_t F, int32_t nfft,
                 double eps, int32_t use_floor, double relative_floor_db, int32_t out_format,
                 const void* twiddle, int32_t dtype, void* y, void* stream);
int dsa_spec_bwd(const void* gy, const void* b, int32_t lb, const void* a, int32_t la, int64_t F,
                 int32_t nfft, double eps, int32_t use_floor, double relative_floor_db,
                 int32_t out_format, const void* twiddle, int32_t dtype, void* gb, void* ga,
                 void* stream);

/* ------------------------------------------------------------------ a5  STFT (fused a1+a2+a3+a4)
 * ShortTimeFourierTransform._forward, stft.py:237-241 = spec(window(frame(x))).
 * x:(B,T), w:(L) window table -> y:(B,N,nfft/2+1) (x2 interleaved for DSA_SPEC_COMPLEX).
 * One kernel: each waveform sample is read from HBM once, frames overlap in LDS. */
int dsa_stft_fwd(const void* x, int64_t B, int64_t T, int32_t L, int32_t P, int32_t nfft,
                 const void* w, const void* twiddle, int32_t center, int32_t zmean,
                 int32_t pad_mode, double eps, int32_t use_floor, double relative_floor_db,
                 int32_t out_format, int32_t dtype, int32_t algo, void* y, void* stream);
/* gy like y -> gx:(B,T); if gw != NULL also gw:(L) (learnable window, stft.py:73-76). */
int dsa_stft_bwd(const void* gy, const void* x, int64_t B, int64_t T, int32_t L, int32_t P,
                 int32_t nfft, const void* w, const void* twiddle, int32_t center, int32_t zmean,
                 int32_t pad_mode, double eps, int32_t use_floor, double relative_floor_db,
                 int32_t out_format, int32_t dtype, int32_t algo, void* gx, void* gw, void* stream);

/* ------------------------------------------------------------------ a6/a7  frequency transform
 * FrequencyTransform._forward freqt.py:141-143 and CoefficientsFrequencyTransform._forward
 * mcep.py:286-288: out:(F,L2) = c:(F,L1) @ A:(L1,L2).  (bwd: gc = gout @ A^T) */
int dsa_freqt_fwd(const void* c, int64_t F, int32_t L1, const void* A, int32_t L2, int32_t dtype,
                  void* out, void* stream);
int dsa_freqt_bwd(const void* gout, int64_t F, int32_t L1, const void* A, int32_t L2,
                  int32_t dtype, void* gc, void* stream);

/* ------------------------------------------------------------------ f1  mel filter bank (SURVEY 8(f) row 1)
 * MelFilterBankAnalysis._forward, fbank.py:306-321.  x:(F,K) power spectrum, H:(K,C) filter weights:
 *   y:(F,C) = glog(max(s @ H, floor)), s = x (use_power) or sqrt(x), glog = log (gamma 0) or (y^gamma-1)/gamma;
 *   E:(F) = log((2 sum_{0<k<K-1} x_k + x_0 + x_{K-1}) / (2 (K-1)))   (E may be NULL).
 * MFCC (mfcc.py:244-256) = this + dsa_freqt_fwd with the DCT-II matrix times the liftering vector. */
int dsa_fbank_fwd(const void* x, int64_t F, int32_t K, const void* H, int32_t C, double floor, double gamma,
                  int32_t use_power, int32_t dtype, void* y, void* E, void* stream);
int dsa_fbank_bwd(const void* gy, const void* gE, const void* x, int64_t F, int32_t K, const void* H, int32_t C,
                  double floor, double gamma, int32_t use_power, int32_t dtype, void* gx, void* stream);
/* MelFrequencyCepstralCoefficientsAnalysis._forward mfcc.py:244-256 in one launch: z:(F,Mo) = glog(max(s H, floor)) W,
 * W:(C,Mo) = DCT-II x truncation x liftering vector (device); E:(F) log energy as dsa_fbank_fwd (may be NULL).  The
 * filter-bank outputs are not materialised; the backward is dsa_freqt_bwd (through W) followed by dsa_fbank_bwd. */
int dsa_fbank_dct_fwd(const void* x, int64_t F, int32_t K, const void* H, int32_t C, const void* W, int32_t Mo, double floor,
                      double gamma, int32_t use_power, int32_t dtype, void* z, void* E, void* stream);
/* The two stages above in ONE launch -- STFT (stft.py:148-152, power format, constant padding) and
 * MelFilterBankAnalysis._forward (fbank.py:306-321, out_format "y") without the (B, N, 257) spectrum ever reaching
 * memory: x:(B,T) -> y:(B, N, C) = glog(max(s @ H, floor)), s = |STFT|^2 + eps (use_power) or its square root.
 * H enters as the per-lane `plan` (device, DSA_FBANK_PLAN_FLOATS float32) that dsa_fbank_scan_plan builds ON THE
 * HOST from H:(257, C) float64 row-major: it exists when every bin feeds at most two ADJACENT channels, in
 * ascending order along the bins (the triangular mel / auditory filters of fbank.py:232-291; C <= 126) -- otherwise
 * DSA_ERR_UNSUPPORTED, and the two-call path above serves the matrix.  The fused kernel covers float32,
 * fft_length 512, frame_length 400, even frame_period (else DSA_ERR_UNSUPPORTED).
 * Its BACKWARD needs no spectrum either: dsa_fbank_bins_bwd turns the cotangent gy:(F, C) of the output and the saved
 * output y:(F, C) into the cotangent g:(F, K) of the filter bank's input -- g[k] = w0 Q(c_k) + w1 Q(c_k + 1),
 * Q(c) = gy_c * dglog/ds at s = glog^-1(y_c), 0 where the floor clamped (fbank.py:312-321 differentiated) -- through the
 * per-bin `table` (device, 4 K float32: {bits of c_k, w0, w1, 0} per bin) that dsa_fbank_bins_plan builds ON THE HOST from
 * H:(K, C) float64 (DSA_ERR_UNSUPPORTED when a bin feeds more than two adjacent channels); g then enters dsa_stft_bwd as
 * the cotangent of the power (use_power) or magnitude spectrum.  float32. */
#define DSA_FBANK_PLAN_FLOATS 2048
int dsa_fbank_scan_plan(const double* H_host, int32_t K, int32_t C, float* plan_host);
int dsa_stft_fbank_fwd(const void* x, int64_t B, int64_t T, int32_t L, int32_t P, int32_t nfft, const void* w,
                       const void* twiddle, int32_t center, double eps, const void* plan, int32_t C, double floor,
                       double gamma, int32_t use_power, int32_t dtype, void* y, void* stream);
int dsa_fbank_bins_plan(const double* H_host, int32_t K, int32_t C, float* table_host);
int dsa_fbank_bins_bwd(const void* gy, const void* y, int64_t F, int32_t K, int32_t C, const void* table, double floor,
                       double gamma, int32_t dtype, void* g, void* stream);

/* ------------------------------------------------------------------ f2  inverse path (SURVEY 8(f) row 2)
 * RealValuedInverseFastFourierTransform ifftr.py:131-142, Unframe unframe.py:164-211, InverseShortTimeFourier-
 * Transform istft.py:186-193.  irfft is the ADJOINT of rfft applied to G_k = c_k / N Y_k (c = 1 at DC and
 * Nyquist, else 2), and overlap-add is the adjoint of framing: the inverse path runs on the backward entries
 * above (dsa_fftr_bwd / dsa_frame_bwd / dsa_stft_bwd with complex cotangents) plus these two helpers.
 *   dsa_irfft_scale: y:(F,nfft/2+1) complex pairs -> out = c_k / nfft * y
 *   dsa_div_rows:    out:(B,T) = x / (d:(T) + eps)   (d = overlap-added squared window, eps = 1e-16) */
int dsa_irfft_scale(const void* y, int64_t F, int32_t nfft, int32_t dtype, void* out, void* stream);
int dsa_div_rows(const void* x, int64_t B, int64_t T, const void* d, double eps, int32_t dtype, void* out, void* stream);
/* InverseShortTimeFourierTransform._forward istft.py:186-193 in one call: y:(B,N,nfft/2+1) complex pairs, N =
 * dsa_num_frames(T, P) -> out:(B,T) = overlap-add(w * irfft(y)[:L]) / (d + d_eps); w:(L) synthesis window, d:(T) the
 * overlap-added squared window (unframe.py:203-205), twiddle as dsa_stft_fwd.  Float32 / fft_length 512 runs on the
 * tuned STFT backward kernels (inverse weights while loading; the division happens as the samples are stored). */
int dsa_istft_fwd(const void* y, int64_t B, int64_t T, int32_t L, int32_t P, int32_t nfft, const void* w,
                  const void* twiddle, int32_t center, const void* d, double d_eps, int32_t dtype, int32_t algo,
                  void* out, void* stream);
/* GriffinLim._forward griffin.py:263-284: the element-wise part of one phase-reconstruction step between
 * z -> dsa_stft_bwd (inverse) -> dsa_stft_fwd (complex) -> t.  y:(B,N,K) power spectrogram; t:(B,Nt,K) complex
 * pairs (Nt >= N, surplus frames dropped; NULL = initial step with phase:(B,N,K) or NULL for zeros);
 * t_prev, d_prev:(B,N,K) complex pairs, updated in place; first != 0 on the first step; z:(B,N,K) complex pairs
 * = sqrt(y + 1e-16) c / (|c| + eps), the next spectrogram to invert. */
int dsa_griffin_update(const void* t, int64_t B, int64_t Nt, int64_t N, int32_t K, const void* y, const void* phase,
                       void* t_prev, void* d_prev, int32_t first, double alpha, double beta, double gamma, double eps,
                       int32_t dtype, void* z, void* stream);

/* ------------------------------------------------------------------ f3  cepstral analysis (SURVEY 8(f) row 3)
 * CepstralAnalysis._forward fftcep.py:116-136 (improved cepstral method).  x:(F, L/2+1) power spectra ->
 * out:(F, M+1).  A:(L/2+1, L/2+1) = c_k cos(2 pi k n / L) (c = 1 at k = 0 and L/2, else 2), device, row-major:
 * every transform of the reference (irfft / hfft / ihfft of even real sequences) is a product with it.
 * masks:(F, n_iter, ceil((L/2+1)/64)) uint64 bit sets of the clamp pattern, written by the forward for the
 * backward (may be NULL when n_iter == 0 or no gradient is needed). */
int dsa_fftcep_fwd(const void* x, int64_t F, int32_t fft_length, int32_t cep_order, const void* A, double accel,
                   int32_t n_iter, int32_t dtype, void* out, void* masks, void* stream);
int dsa_fftcep_bwd(const void* gout, const void* x, int64_t F, int32_t fft_length, int32_t cep_order, const void* A,
                   double accel, int32_t n_iter, const void* masks, int32_t dtype, void* gx, void* stream);

/* ------------------------------------------------------------------ a8-a10  mel-cepstral analysis
 * MelCepstralAnalysis._forward, mcep.py:189-224 (incl. symmetric_toeplitz / hankel,
 * utils/private.py:291-302, and the torch.linalg.solve call at mcep.py:221).
 * X:(F,nfft/2+1) power spectrum -> mc:(F,M+1).  The host composes the reference's linear maps
 * once per configuration (float64, then cast):
 *   G:(H+1,M+1)  = irfft-with-halved-ends  o freqt          (mcep.py:204-207)
 *   D:(M+1,H+1)  = ifreqt o Re(rfft(., nfft))               (mcep.py:210-211)
 *   E:(H+1,2M+1) = irfft o rfreqt                           (mcep.py:214-215)
 *   alpha_vec:(M+1) = (-alpha)^i                            (mcep.py:179-181)
 * so that one Newton step is  d = mc D ; e = exp(log X - 2 d) ; rt = e E ;
 * mc += solve(T(rt[:M+1]) + H(rt), rt[:M+1] - alpha_vec).
 * mc_hist: NULL or (n_iter+1, F, M+1) receiving mc after 0..n_iter steps (saved for backward).
 * images / scratch: see Conventions.  The tuned gfx950 kernel (float32, fft_length 512, cep_order 24) consumes G, D, E
 * as binary16 hi/lo operand images in matrix-core lane order: dsa_mcep_images_bytes() is their size (0 when the
 * configuration has no tuned kernel: images may then be NULL) and dsa_mcep_prepare() writes them -- once per
 * configuration, what MelCepstralAnalysis._precompute (mcep.py:133-187) is to the reference.  With
 * DSA_ALGO_AUTO the tuned kernel runs iff the configuration allows it AND images and scratch are given. */
int64_t dsa_mcep_images_bytes(int32_t nfft, int32_t M, int32_t dtype);
int dsa_mcep_prepare(const void* G, const void* D, const void* E, int32_t nfft, int32_t M, int32_t dtype,
                     void* images, void* stream);
int dsa_mcep_fwd(const void* X, int64_t F, int32_t nfft, int32_t M, int32_t n_iter, const void* G,
                 const void* D, const void* E, const void* alpha_vec, int32_t dtype, int32_t algo,
                 const void* images, void* scratch, void* mc, void* mc_hist, void* stream);
/* Gain normalisation of generalized cepstra (gnorm.py:102-112) and its inverse (ignorm.py:99-109), forward, one launch each:
 *   inverse = 0:  x:(F,n) -> (K, x1 / (1 + gamma x0)),  K = (1 + gamma x0)^(1/gamma)   (gamma = 0: (exp x0, x1))
 *   inverse = 1:  y:(F,n) -> ((K^gamma - 1) / gamma, y1 K^gamma)                          (gamma = 0: (log K, y1)) */
int dsa_gnorm_fwd(const void* x, int64_t F, int32_t n, double gamma, int32_t inverse, int32_t dtype, void* out, void* stream);
/* The gain of a Newton step of the mel-generalized analysis joined to its coefficients (mgcep.py:213-215, 221, 231-233):
 * b:(F, M+1) = (sqrt(r_0 + gamma sum_m r_{m+1} b_eps_m), b_join),  r:(F, M+1), b_eps, b_join:(F, M) (the same rows at gamma = -1,
 * the coefficients before / after the step's update otherwise). */
int dsa_mgcep_gain(const void* r, const void* b_eps, const void* b_join, int64_t F, int32_t M, double gamma, int32_t dtype, void* b,
                   void* stream);
/* The solve-and-update of a Newton step of MelCepstralAnalysis (mcep.py:216-222) at a geometry without a tuned kernel:
 * mc_out:(F,n) = mc_in + solve(T(rt[:, :n]) + H(rt), rt[:, :n] - alpha_vec), rt:(F, 2n-1), n = cep_order + 1 in [2, 55], float32.
 * 16 systems per wave on the float32 matrix instruction, no pivoting; a system that meets a non-positive pivot is re-solved with
 * row pivoting by a second launch (csrc/thsolve_quad.hip).  mc_out may be mc_in. */
int dsa_mcep_newton_update(const void* rt, int64_t F, int32_t n, const void* alpha_vec, int32_t dtype, const void* mc_in,
                           void* mc_out, void* stream);
/* Its backward.  mc_in = NULL in the call above leaves the solution s alone in mc_out; with gs:(F,n) the cotangent of s this writes
 * grt:(F, 2n-1), the cotangent of rt: u = A^-1 gs on the same batched solve (A is symmetric; u:(F,n) is caller workspace), then
 * grt[k] = -sum_{i+j=k} u_i s_j - [k<n] sum_{|i-j|=k} u_i s_j + [k<n] u_k   (Hankel part, Toeplitz part, right-hand side). */
int dsa_mcep_newton_update_bwd(const void* gs, const void* rt, const void* sol, int64_t F, int32_t n, int32_t dtype, void* u,
                               void* grt, void* stream);
/* The spectral half of the same Newton step (mcep.py:210-215) in one launch:
 *   rt:(F, 2n-1) = exp(logx - 2 mc D) E,   logx:(F,K) = log X, mc:(F,n), D:(n x K, row stride ldd), E:(K x (2n-1), row stride lde),
 * n = cep_order + 1 in [3, 55], K >= 4, float32.  e = exp(.) is produced chunk by chunk in the operand layout of the second
 * product (v_mfma_f32_16x16x4_f32 for both) and never reaches memory (csrc/rows_gemm.hip:mcep_resid_mfma_kernel). */
int dsa_mcep_newton_resid(const void* logx, int64_t F, int32_t K, const void* mc, int32_t n, const void* D, int32_t ldd,
                          const void* E, int32_t lde, int32_t dtype, void* rt, void* stream);
/* (0.1.9) The same launch with both products as 3-term binary16 splits on the matrix pipe (csrc/mcep_resid_f16.h: 12 + 21 binary16
 * products per 32 bins and 16 frames at order 49 instead of 82 float32 ones): `images` = dsa_mcep_resid_images_bytes(K, n) bytes of
 * caller-owned device memory filled ONCE per configuration by dsa_mcep_resid_prepare from D (n x K) and E (K x 2n - 1); logx holds
 * natural logarithms as for dsa_mcep_newton_resid. */
int64_t dsa_mcep_resid_images_bytes(int32_t K, int32_t n);
int dsa_mcep_resid_prepare(const void* D, int32_t ldd, const void* E, int32_t lde, int32_t K, int32_t n, int32_t dtype, void* images,
                           void* stream);
/* (0.2.0) ALL n_iter Newton steps of mcep.py:208-222 in ONE persistent launch (csrc/mcep_big_f16.h): per step the two products of
 * dsa_mcep_newton_resid_h (same images, bit-identical rt) and the solve-and-update of dsa_mcep_newton_update, rt and mc staying on
 * chip; mc_in:(F, n) the start (mc0 = logx G), mc_out:(F, n) (may be mc_in).  Orders n - 1 in 32 .. 54 (the 48 kHz set-ups fft_length
 * 2048 / order 49 and 1024 / order 34 among them); DSA_ERR_UNSUPPORTED otherwise -- alternate dsa_mcep_newton_resid_h and dsa_mcep_newton_update then. */
int dsa_mcep_newton_steps(const void* logx, int64_t F, int32_t K, const void* mc_in, int32_t n, const void* images, const void* alpha_vec,
                          int32_t n_iter, int32_t dtype, void* mc_out, void* stream);
int dsa_mcep_newton_resid_h(const void* logx, int64_t F, int32_t K, const void* mc, int32_t n, const void* images, int32_t dtype,
                            void* rt, void* stream);
/* (0.2.1) The ADJOINT of dsa_mcep_newton_resid_h -- what autograd derives from mcep.py:210-215 -- in one launch on the binary16 matrix
 * pipe (csrc/mcep_resid_bwd_f16.h), orders n - 1 in 32 .. 54 (dsa_mcep_resid_bwd_images_bytes returns 0 otherwise: keep the composed
 * gradient there): given grt:(F, 2n - 1), the cotangent of rt = exp(logx - 2 mc D) E,
 *   glogx:(F, K) += ebar * e,   gmc:(F, n) = -2 (ebar * e) D^T,   ebar = grt E^T,  e = exp(logx - 2 mc D) recomputed from the iterate
 * (glogx is read-modify-written: the caller zeroes it before the first step of the reverse sweep; gmc is overwritten).  `images` =
 * dsa_mcep_resid_bwd_images_bytes(K, n) bytes of caller-owned device memory filled ONCE per configuration by
 * dsa_mcep_resid_bwd_prepare from D (n x K) and E (K x 2n - 1).  With dsa_mcep_newton_update_bwd (the solve on the cotangent and
 * the diagonal sums: grt) this is a Newton step's whole backward: two launches, no intermediate of the forward kept but the iterates,
 * the rt rows and the solutions. */
int64_t dsa_mcep_resid_bwd_images_bytes(int32_t K, int32_t n);
int dsa_mcep_resid_bwd_prepare(const void* D, int32_t ldd, const void* E, int32_t lde, int32_t K, int32_t n, int32_t dtype, void* images,
                               void* stream);
int dsa_mcep_newton_resid_h_bwd(const void* logx, int64_t F, int32_t K, const void* mc, int32_t n, const void* grt, const void* images,
                                int32_t dtype, void* glogx, void* gmc, void* stream);
/* (0.2.2) The sum over the Newton steps that dsa_mcep_newton_resid_h_bwd accumulates into glogx, formed in ONE pass over the bins after
 * the reverse sweep instead (autograd of mcep.py:210-215 summed over mcep.py:208-222's iterations):
 *   glogx[f, k] = sum_s (sum_j grts[s][f][j] E[k][j]) * exp(logx[f][k] - 2 sum_c mcs[s][f][c] D[c][k])
 * mcs:(n_iter, F, n) the iterates the steps started from, grts:(n_iter, F, 2n - 1) the cotangents of their rt rows
 * (dsa_mcep_newton_update_bwd's `grt`, kept per step), images of dsa_mcep_resid_bwd_prepare; glogx:(F, K) is WRITTEN.  The sweep's
 * launches then pass glogx = NULL to dsa_mcep_newton_resid_h_bwd (a step moves the (F, K) array once instead of three times).  The
 * steps are summed in the sweep's order on the same values: bit-identical to the in-place accumulation.  DSA_ERR_UNSUPPORTED
 * (no error text): orders outside 32 .. 54, or n_iter above what one workgroup's LDS holds (12 at orders >= 48, 15 below) -- the
 * caller keeps the in-place accumulation. */
int dsa_mcep_newton_glogx_h(const void* logx, int64_t F, int32_t K, const void* mcs, int32_t n, const void* grts, int32_t n_iter,
                            const void* images, int32_t dtype, void* glogx, void* stream);
/* General float32 row product on the matrix instruction, for shapes the kernels behind dsa_freqt_fwd / _bwd do not cover (rows
 * of 512 values and more: the 1025-bin products of the 48 kHz set-ups of utils/public.py:22-104) and for the Newton step of
 * MelCepstralAnalysis (mcep.py:203-215) at geometries without a tuned kernel:
 *   out:(F,N) = op_out( op_in(c):(F,K) x B:(K,N) ),  B = A (K x N, row stride lda) or, with DSA_ROWS_TRANS, A^T (A: N x K, stride lda)
 *   DSA_ROWS_PRO_LOG    op_in = log          (mcep.py:203 feeding :204-207)
 *   DSA_ROWS_EPI_EXPSUB op_out(v) = exp(aux - 2 v), aux:(F,N) with row stride ldaux   (mcep.py:210-212)
 * Exact float32 products, float32 accumulation (v_mfma_f32_16x16x4_f32).  ldo: row stride of out. */
#define DSA_ROWS_PRO_LOG 1
#define DSA_ROWS_EPI_EXPSUB 2
#define DSA_ROWS_TRANS 4
int dsa_rows_gemm(const void* c, int64_t F, int32_t K, const void* A, int32_t lda, int32_t N, int32_t flags, const void* aux,
                  int32_t ldaux, int32_t dtype, void* out, int32_t ldo, void* stream);
/* element-wise companions of the same analysis when a gradient is wanted (the fused forms keep no operands):
 *   op 0: o0 = log(a)            backward (backward = 1): o0 = gy / a
 *   op 1: o0 = exp(a - 2 b)      backward: a = the saved OUTPUT y, o0 = gy y (cotangent of a), o1 = -2 gy y (cotangent of b)   */
int dsa_rows_ew(int32_t op, int32_t backward, const void* a, const void* b, const void* gy, int64_t n, int32_t dtype, void* o0,
                void* o1, void* stream);
/* ShortTimeFourierTransform._forward (stft.py:237-241: frame, window, rfft, |.|^2 + eps) feeding
 * MelCepstralAnalysis._forward (mcep.py:189-224) in ONE launch: x:(B,T) -> mc:(B N, M+1), N = (T-1)/P + 1, without the
 * (B, N, nfft/2+1) power spectrogram's round trip through memory (320 + 100 bytes per frame instead of 1348 + 1128).  The
 * persistent mel-cepstral wave computes the 16 spectra of its tile itself, with the instructions of the packed STFT kernel
 * (bit-identical power values), and takes log2 straight into the registers the Newton iteration keeps them in.
 * Covers float32, frame_length 400, fft_length 512, cep_order 24, power format, constant padding, no zmean / relative floor
 * (else DSA_ERR_UNSUPPORTED: call dsa_stft_fwd and dsa_mcep_fwd).  window:(L), twiddle:(nfft,2), G/D/E/alpha_vec/images/
 * scratch/algo flags as dsa_mcep_fwd; mc_hist: NULL or (n_iter+1, B N, M+1); X_out: NULL or (B N, nfft/2+1) receiving the
 * power spectrogram as a side product (what dsa_mcep_bwd needs when a gradient is wanted). */
/* (0.2.0) The same launch with the options of ShortTimeFourierTransform it covers beyond the plain configuration (stft.py:86-104):
 * zmean (frame.py:139-140), pad_mode (DSA_PAD_*, frame.py:130-137), the relative floor in dB (spec.py:174-176); power format only.
 * Options run own instantiations of the kernel: the plain configuration's code is untouched. */
int dsa_stft_mcep_opts_fwd(const void* x, int64_t B, int64_t T, int32_t L, int32_t P, int32_t nfft, const void* window,
                           const void* twiddle, int32_t center, int32_t zmean, int32_t pad_mode, double eps, int32_t use_floor,
                           double relative_floor_db, int32_t M, int32_t n_iter, const void* G, const void* D, const void* E,
                           const void* alpha_vec, int32_t dtype, int32_t algo, const void* images, void* scratch, void* mc,
                           void* mc_hist, void* X_out, void* stream);
int dsa_stft_mcep_fwd(const void* x, int64_t B, int64_t T, int32_t L, int32_t P, int32_t nfft, const void* window,
                      const void* twiddle, int32_t center, double eps, int32_t M, int32_t n_iter, const void* G,
                      const void* D, const void* E, const void* alpha_vec, int32_t dtype, int32_t algo,
                      const void* images, void* scratch, void* mc, void* mc_hist, void* X_out, void* stream);
/* gradient of the UNROLLED n_iter-step iteration (what autograd gives the reference).
 * gmc:(F,M+1), X, mc_hist as saved by the forward -> gX:(F,nfft/2+1). */
int dsa_mcep_bwd(const void* gmc, const void* X, const void* mc_hist, int64_t F, int32_t nfft,
                 int32_t M, int32_t n_iter, const void* G, const void* D, const void* E,
                 const void* alpha_vec, int32_t dtype, int32_t algo, const void* images, void* scratch,
                 void* gX, void* stream);

/* ------------------------------------------------------------------ f3  mel-generalized cepstral analysis (SURVEY 8(f) row 3)
 * The Toeplitz-plus-Hankel solve of MelGeneralizedCepstralAnalysis.forward, mgcep.py:226-229 (symmetric_toeplitz /
 * hankel of utils/private.py:291-302, torch.linalg.solve): g:(F,n) = solve(T(p) + H(q), r), p:(F,n) the first
 * column of the Toeplitz part, q:(F,2n-1) the anti-diagonals of the Hankel part, r:(F,n); n <= 64, row-pivoted
 * (float32, n = 24: 16 systems per wave without pivoting, as the mel-cepstral kernels solve theirs -- the matrix is positive
 * definite for the analysis' gamma in [-1, 0]; a system whose elimination meets a non-positive pivot is re-solved with row
 * pivoting by a second launch, so arbitrary symmetric systems get the pivoted answer the reference's LAPACK call gives).
 * Backward: cotangent gg:(F,n) -> gp, gq, gr.  The other stages of the analysis are row products against matrices
 * the host composes (dsa_freqt_fwd) around pointwise spectrum arithmetic (modules/mgcep.py). */
int dsa_thsolve_fwd(const void* p, const void* q, const void* r, int64_t F, int32_t n, int32_t dtype, void* g,
                    void* stream);
/* The pointwise spectrum arithmetic of one Newton step, mgcep.py:199-209 (gamma in [-1, 0), not 0), in one pass:
 * x:(F,K) power spectra, b1:(F,M) the current coefficients b[1:], Cr, Ci:((M+1),K) the composed cfreqt -> rfft
 * matrices (tables.mgcep_matrices; row 0 is not read: b[0] = 0 there) -> out:(5,F,K) = pp, qq (X^2 - Y^2), qq 2XY,
 * pp X, pp Y -- the inputs of the row products against Pr, Qr, Qi, Rr, Ri (dsa_freqt_fwd).  Forward only: with a
 * gradient needed the module composes the same arithmetic from differentiable operators.  M <= 64. */
int dsa_mgcep_spectra(const void* x, const void* b1, int64_t F, int32_t fft_length, int32_t M, const void* Cr,
                      const void* Ci, double gamma, int32_t dtype, void* out, void* stream);
int dsa_thsolve_bwd(const void* gg, const void* p, const void* q, const void* g, int64_t F, int32_t n, int32_t dtype,
                    void* gp, void* gq, void* gr, void* stream);
/* The Newton update of mgcep.py:226-230 in one call: b_out = b_in + solve(symmetric_toeplitz(p) + hankel(q), r) with the
 * right-hand side read in place from a wider vector: row f of r starts at r + f * r_stride + r_offset (the step's (F, n + 1)
 * vector with r_offset = 1).  Order 24 in float32 (DSA_ERR_UNSUPPORTED otherwise); b_in and b_out must not alias. */
int dsa_thsolve_update_fwd(const void* p, const void* q, const void* r, int64_t r_stride, int64_t r_offset, int64_t F,
                           int32_t n, int32_t dtype, const void* b_in, void* b_out, void* stream);
/* The same step's spectrum arithmetic AND its five row products in one launch (mgcep.py:199-220; float32, fft_length 512,
 * cep_order <= 24, gamma in [-1, 0)): x:(F,257), b1:(F,M) -> pt:(F,M) = pp Pr[:, :M], qt:(F,2M-1) = (1 + gamma)(.. Qr[:, 2:] + .. Qi[:, 2:]),
 * r:(F,M+1) = pp X Rr + pp Y Ri -- the operands of dsa_thsolve_fwd.  The five spectra never exist in memory (dsa_mgcep_spectra writes
 * them for the float64 / other-size path).  `images`: 17 x 3840 float32, the matrices in matrix-instruction lane order, built by the
 * caller once per configuration (layout: csrc/mgc.hip, mgcep_step_kernel; diffsptk_amd.utils.tables.mgcep_step_images).  Forward only. */
int dsa_mgcep_step(const void* x, const void* b1, int64_t F, int32_t fft_length, int32_t M, double gamma, const void* images,
                   int32_t dtype, void* pt, void* qt, void* r, void* stream);
/* (0.1.9) dsa_mgcep_step_bwd on the binary16 matrix pipe (cep_order 24 / fft_length 512 / float32; csrc/mgcep_step_f16.h): same
 * arguments, `images_bwd_h`: 9 x 22528 binary16 (diffsptk_amd.utils.tables.mgcep_step_bwd_h_images).  66 binary16 products per 32 bins and
 * 16 frames instead of 144 float32 ones. */
int dsa_mgcep_step_bwd_h(const void* x, const void* b1, const void* gpt, const void* gqt, const void* gr, int64_t F,
                         int32_t fft_length, int32_t M, double gamma, const void* images_bwd_h, int32_t dtype, const void* gx_in,
                         void* gx, void* gb1, void* stream);
/* (0.1.9) The WHOLE Newton step in one launch (mgcep.py:199-230; float32, fft_length 512, cep_order 24, gamma in (-1, 0)): the spectrum
 * arithmetic, the five row products as 3-term binary16 splits on the matrix pipe, the 24 x 24 Toeplitz-plus-Hankel solve (block
 * elimination, pivoted re-solve for systems that are not positive definite) and the update: x:(F,257), b1:(F,24) ->
 * b1_out:(F,24) = b1 + solve(toeplitz(pt) + hankel(qt), r[1:]) (b1_out may be b1), r:(F,25) (what the gain of mgcep.py:221 reads).
 * `images_h`: 9 x 16384 binary16 followed by 240 float32 (the matrices at the Nyquist bin), built by the caller once per configuration
 * (diffsptk_amd.utils.tables.mgcep_step_h_buffer; layout: csrc/mgcep_step_f16.h).  `pt`:(F,24), `qt`:(F,47): NULL, or where the system's two generators are kept for a graph (the backward is
 * dsa_thsolve_bwd on (pt, qt, b1_out - b1) followed by dsa_mgcep_step_bwd).  Replaces dsa_mgcep_step + dsa_thsolve_update_fwd (95 + 32 us
 * per 51 200 frames: 80).  `n_steps` >= 1 Newton steps run in the ONE launch (a frame's iteration depends on the frame alone: the
 * coefficients stay in LDS between the steps); r, pt, qt are the LAST step's, `b1_prev`:(F,24) (or NULL) the last step's input. */
int dsa_mgcep_step_solve(const void* x, const void* b1, int64_t F, int32_t fft_length, int32_t M, double gamma, const void* images_h,
                         int32_t dtype, void* b1_out, void* r, void* pt, void* qt, int32_t n_steps, void* b1_prev, void* stream);
/* Backward of dsa_mgcep_step in one launch: cotangents gpt:(F,M), gqt:(F,2M-1), gr:(F,M+1) -> gx:(F,L/2+1) (+ gx_in when not
 * NULL: the spectrum enters every Newton step, so the steps' contributions accumulate; gx_in may be gx) and gb1:(F,M).
 * `images_bwd`: 17 x 4608 float32 built by the caller (diffsptk_amd/utils/tables.py:mgcep_step_bwd_images). */
int dsa_mgcep_step_bwd(const void* x, const void* b1, const void* gpt, const void* gqt, const void* gr, int64_t F,
                       int32_t fft_length, int32_t M, double gamma, const void* images_bwd, int32_t dtype, const void* gx_in,
                       void* gx, void* gb1, void* stream);
/* GeneralizedCepstrumToGeneralizedCepstrum._forward, mgc2mgc.py:333-361 (the FFT formulation of the generalized cepstral
 * transformation), in ONE launch: c1:(F,n_in) gain-normalised generalized cepstra of in_gamma -> c2:(F,out_order+1) of
 * out_gamma through fft(c01, n_fft) -> (1 + g1 C)^(1/g1) -> (|s|^g2 cos(g2 angle s) - 1) / g2 -> ifft(.).real, n_fft a power of
 * two (the row lives in LDS: 8 n_fft bytes in float32, 16 n_fft in float64, <= 150 KB).  `twiddle`: (n_fft, 2) as for dsa_fftr_fwd.
 * `flags` folds the per-row scalar steps MelGeneralizedCepstrumToMelGeneralizedCepstrum wraps around it (mgc2mgc.py:217-300):
 * 1 = gain normalisation with in_gamma before (gnorm.py:99-109), 2 = inverse gain normalisation with out_gamma after
 * (ignorm.py:99-109), 4 = c[1:] *= out_gamma (GammaMultiplication), 8 = c[0] = c[0] out_gamma + 1 (ZerothGammaMultiplication).
 * Forward only: with a gradient needed the module composes dsa_fftr_fwd / element-wise operators / the inverse transform.
 * This is what mgc2mgc (gamma conversion), mgc2sp and the MLSA filter's impulse responses (mglsadf.py:389-527) run on. */
int dsa_gc2gc_fwd(const void* c1, int64_t F, int32_t n_in, int32_t out_order, double in_gamma, double out_gamma,
                  int32_t nfft, const void* twiddle, int32_t flags, int32_t dtype, void* c2, void* stream);
/* Backward of dsa_gc2gc_fwd with flags = 0, one launch: the row c1:(F, n_in) and the cotangent g2:(F, out_order + 1) of c2 ->
 * gc1:(F, n_in).  n_fft a power of two; float32 up to 8192 points, float64 up to 4096 (the three half-length transforms and the
 * half spectrum live in LDS). */
int dsa_gc2gc_bwd(const void* c1, const void* g2, int64_t F, int32_t n_in, int32_t out_order, double in_gamma, double out_gamma,
                  int32_t nfft, const void* twiddle, int32_t dtype, void* gc1, void* stream);

/* ------------------------------------------------------------------ f4  time-variant all-zero filter (SURVEY 8(f) row 4)
 * AllZeroDigitalFilter._forward_efficient, zerodf.py:207-243: the FIR core of the multi-stage / single-stage MLSA filter
 * (mglsadf.py:254-527).  x:(B,T), b:(B,N,M+1) with T = N P -> y:(B,T),
 *   y[t] = sum_k h_t[k] x[t - k + zeroth_index],  h_t = lerp(b[t / P], b[min(t / P + 1, N - 1)], (t % P) / P);
 * ignore_gain divides by the interpolated gain tap (b[.][0], or b[.][M] when zeroth_index = M).
 * Backward: gy, and the forward's x, b, y -> gx:(B,T) and / or gb:(B,N,M+1) (either may be NULL). */
int dsa_zerodf_fwd(const void* x, const void* b, int64_t B, int64_t T, int32_t M, int32_t P, int32_t zeroth_index,
                   int32_t ignore_gain, int32_t dtype, void* y, void* stream);
int dsa_zerodf_bwd(const void* gy, const void* x, const void* b, const void* y, int64_t B, int64_t T, int32_t M, int32_t P,
                   int32_t zeroth_index, int32_t ignore_gain, int32_t dtype, void* gx, void* gb, void* stream);
/* One Taylor stage of the multi-stage MLSA filter (mglsadf.py:356-365: x <- F x / i, y <- y + x) in one launch:
 *   y = scale * zerodf(x; b)   (y may be NULL when only the sum is wanted: the last stage),
 *   ysum = acc + y             (acc and ysum both NULL or both given; they may be the same buffer).
 * Rounded exactly like the three separate operations.  Needs P % 4 == 0 and M >= 16 (DSA_ERR_UNSUPPORTED otherwise:
 * use dsa_zerodf_fwd and element-wise launches). */
int dsa_zerodf_taylor_fwd(const void* x, const void* b, int64_t B, int64_t T, int32_t M, int32_t P, int32_t zeroth_index,
                          double scale, const void* acc, int32_t dtype, void* y, void* ysum, void* stream);
/* Backward of one Taylor stage (x_i = F x_{i-1} / i, y = sum x_i): with G the cotangent that reaches x_i, one call gives
 *   G_out = gy + scale * F^T G      (the cotangent that reaches x_{i-1}; gy: the cotangent of y; G_out must not alias G),
 *   gb   += scale * dF(x_{i-1})^T G (accumulated over the stages: the caller zeroes gb once; may be NULL).
 * Same shape limits as dsa_zerodf_taylor_fwd. */
int dsa_zerodf_taylor_bwd(const void* G, const void* x, const void* b, int64_t B, int64_t T, int32_t M, int32_t P,
                          int32_t zeroth_index, double scale, const void* gy, int32_t dtype, void* G_out, void* gb, void* stream);

/* ------------------------------------------------------------------ f5  time-variant all-pole filter (0.2.4)
 * AllPoleDigitalFilter._forward, poledf.py:117-140 (the reference delegates the recursion to torchlpc.sample_wise_lpc): the LPC
 * synthesis filter.  x:(B,T), a:(B,N,M+1) with T = N P, a row [K, a_1 .. a_M] -> y:(B,T), zero initial state:
 *   c_t = lerp(a[t / P], a[min(t / P + 1, N - 1)], (t % P) / P),  g_t = c_t[0] (1 with ignore_gain),
 *   y[t] = g_t x[t] - sum_{k=1..M} c_t[k] y[t - k].
 * Backward: gy, and the forward's x, a, y -> the adjoint state u:(B,T) (always written: a caller-owned buffer, the library owns no
 * device memory), gx:(B,T) and / or ga:(B,N,M+1) (either may be NULL; x and y are only read for ga):
 *   u[t] = gy[t] - sum_{k=1..M} c_{t+k}[k] u[t + k],  gx[t] = g_t u[t],
 *   dc_t[k] = -u[t] y[t - k] (k >= 1),  dc_t[0] = u[t] x[t] (0 with ignore_gain),  ga = the adjoint of the interpolation of dc.
 * One wave per utterance for 1 <= M <= 63 (a row window of 63 / P + 3 frames of M + 1 values within 512); other shapes take a
 * plain one-thread-per-utterance kernel.  0 <= M <= DSA_POLEDF_MAX_ORDER. */
#define DSA_POLEDF_MAX_ORDER 4096
int dsa_poledf_fwd(const void* x, const void* a, int64_t B, int64_t T, int32_t M, int32_t P, int32_t ignore_gain, int32_t dtype,
                   void* y, void* stream);
int dsa_poledf_bwd(const void* gy, const void* x, const void* a, const void* y, int64_t B, int64_t T, int32_t M, int32_t P,
                   int32_t ignore_gain, int32_t dtype, void* u, void* gx, void* ga, void* stream);

/* ------------------------------------------------------------------ f6  perceptual linear prediction after the filter bank (0.2.5)
 * PerceptualLinearPredictiveCoefficientsAnalysis._forward, plp.py:313-320, from `y, E = fbank(x)` on (plp.py:314), with
 * levdur.py:114-127 (eps = 0) and mgc2mgc.py:207-300 (in_gamma = -1, in_norm, in_mul -> gamma 0: lpc2c).  y:(F,C) log filter-bank
 * outputs, E:(F) log energy (read only when out_format carries it; may be NULL otherwise) -> out:(F, Mo), Mo = M + {0, 1, 1, 2}
 * for out_format 0 y, 1 yE, 2 yc, 3 ycE:
 *   v_c = (exp(y_c) q_c)^cf,  u = [v_0, v, v_{C-1}],  r_k = sum_n u_n Q[n][k] (hfft(u, norm="forward")[:M+1]),  [K, a] = levdur(r),
 *   c_0 = log K,  c_m = sum_{j=0..N/2} w_j log|1 + sum_l a_l e^{-2 pi i j l / N}| cos(2 pi j m / N)  (the reference's aliased
 *   N-point sum),  c *= lifter,  out row = [c_1 .. c_M] (+ c_0) (+ E).
 * table: the packed float64-built constants in the data's dtype (utils/tables.py: plp_table), J = N/2 + 1:
 *   [q (C) | Q (C+2, M+1) | cos (M+1, J) | sin (M+1, J) | w (J) = -(2/N) {1, 2, .., 2, (1)} | lifter (M+1)].
 * save:(F, M+1) (may be NULL) receives [K, a] for the backward.  Backward: gout:(F, Mo), the forward's y and save -> gy:(F,C) (the
 * cotangent of the filter-bank outputs, for dsa_fbank_bwd / dsa_fbank_bins_bwd) and gE:(F) (may be NULL; the pass-through of E's
 * column, 0 without one).  One wave per frame: a frame's bits do not depend on F.  0 <= M <= DSA_PLP_MAX_ORDER, C > M, N > M + 1;
 * float32 and float64; F = 0 is a no-op; no allocation, no host synchronisation. */
#define DSA_PLP_MAX_ORDER 62
int dsa_plp_fwd(const void* y, const void* E, int64_t F, int32_t C, int32_t M, int32_t N, double compression_factor,
                int32_t out_format, const void* table, int32_t dtype, void* out, void* save, void* stream);
int dsa_plp_bwd(const void* gout, const void* y, const void* save, int64_t F, int32_t C, int32_t M, int32_t N,
                double compression_factor, int32_t out_format, const void* table, int32_t dtype, void* gy, void* gE, void* stream);

/* ------------------------------------------------------------------ f7  pseudo-QMF subband analysis and synthesis (0.2.6)
 * PseudoQuadratureMirrorFilterBankAnalysis.forward, pqmf.py:250-258 (ConstantPad1d, ReplicationPad1d and conv1d with K output
 * channels), with the Decimation that may follow it (decimate.py:88-93, x[..., start::period]) folded in; and
 * PseudoQuadratureMirrorFilterBankSynthesis.forward, ipqmf.py:132-141, with the Interpolation that may precede it
 * (interpolate.py:85-96, zeros + index_copy_) folded in.  f:(K, M+1) are the filters in the reference's stored, time-flipped layout
 * (its conv1d weights, (K,1,M+1) / (1,K,M+1), without the unit axis):
 *   dsa_pqmf_fwd   x:(B,T) -> y:(B,K,Tout), Tout = len(range(start, T, period)):
 *                  y[b,k,m] = sum_i f[k,i] xp[b, start + m period + i],  xp = dl zeros | x | dr copies of x[T-1]
 *                  (dl, dr) = (M/2, M/2) for even M, ((M+1)/2, (M-1)/2) for odd M;  only the kept outputs are computed.
 *   dsa_ipqmf_fwd  y:(B,K,T) -> x:(B,Tu), Tu = T up + start:  x[b,t] = sum_k sum_i f[k,i] yp[b,k,t + i],  yp = dl zeros | yu |
 *                  dr copies of yu[Tu-1], yu = y zero-stuffed (y[b,k,m] at start + m up), (dl, dr) = ((M-1)/2, (M+1)/2) for odd M;
 *                  only the taps on non-zero samples are evaluated and yu is never written.
 *   (period, start) = (1, 0) and (up, start) = (1, 0) are the plain modules.
 * Backward: dsa_pqmf_bwd gy:(B,K,Tout) -> gx:(B,T) (the replicate pad's gradients summed into x[T-1]) and / or gf:(K,M+1);
 * dsa_ipqmf_bwd gx:(B,Tu) -> gy:(B,K,T) (at the kept positions only) and / or gf.  Either output may be NULL.  gf needs the forward's
 * input (x / y) and `work`, a caller-owned workspace of B K (M+1) elements of the dtype: per-utterance partials, each a sum over
 * time in ascending order, then summed in a fixed order -- no atomics, the same bits run to run.
 * Each output element is one fma chain in a fixed tap order whatever the tiling: a row's bits do not depend on B, and the folded
 * routes give the bits of the module chain for finite data (a skipped tap is an exact zero product).  Tuned kernels for K <= 8,
 * M <= 127, period / up <= 16, generic ones otherwise; float32 and float64; no allocation, no host synchronisation.
 * 1 <= K <= DSA_PQMF_MAX_BANDS, 2 <= M <= DSA_PQMF_MAX_ORDER. */
#define DSA_PQMF_MAX_BANDS 1024
#define DSA_PQMF_MAX_ORDER 2047
int dsa_pqmf_fwd(const void* x, const void* f, int64_t B, int64_t T, int32_t K, int32_t M, int32_t period, int32_t start, int32_t dtype,
                 void* y, void* stream);
int dsa_pqmf_bwd(const void* gy, const void* x, const void* f, int64_t B, int64_t T, int32_t K, int32_t M, int32_t period, int32_t start,
                 int32_t dtype, void* gx, void* gf, void* work, void* stream);
int dsa_ipqmf_fwd(const void* y, const void* f, int64_t B, int64_t T, int32_t K, int32_t M, int32_t up, int32_t start, int32_t dtype,
                  void* x, void* stream);
int dsa_ipqmf_bwd(const void* gx, const void* y, const void* f, int64_t B, int64_t T, int32_t K, int32_t M, int32_t up, int32_t start,
                  int32_t dtype, void* gy, void* gf, void* work, void* stream);
/* Interpolation._forward, interpolate.py:85-96, over the (outer, T, inner) view of a contiguous tensor (any `dim`): y:(outer, T period
 * + start, inner) is zero except y[o, start + n period, i] = x[o, n, i] (every element written: no separate zero fill).  Backward:
 * the strided gather gx[o, n, i] = gy[o, start + n period, i]. */
int dsa_interpolate_fwd(const void* x, int64_t outer, int64_t T, int64_t inner, int32_t period, int32_t start, int32_t dtype, void* y,
                        void* stream);
int dsa_interpolate_bwd(const void* gy, int64_t outer, int64_t T, int64_t inner, int32_t period, int32_t start, int32_t dtype, void* gx,
                        void* stream);

/* ------------------------------------------------------------------ a11  autocorrelation
 * Autocorrelation._forward, acorr.py:110-120.  x:(F,L) -> r:(F,M+1).  Computed as direct lag
 * sums (the reference's irfft(|rfft(x, L+M)|^2) is the same quantity: no circular wrap). */
int dsa_acorr_fwd(const void* x, int64_t F, int32_t L, int32_t M, int32_t out_format, int32_t dtype,
                  void* r, void* stream);
int dsa_acorr_bwd(const void* gr, const void* x, int64_t F, int32_t L, int32_t M, int32_t out_format,
                  int32_t dtype, void* gx, void* stream);

/* ------------------------------------------------------------------ a12  Levinson-Durbin
 * LevinsonDurbin._forward, levdur.py:113-127: a = solve(toeplitz(r[:M]) + eps I, -r[1:]),
 * K = sqrt(sum r[1:] a + r[0]); out:(F,M+1) = [K, a].  Solved by the Levinson recursion on
 * (r0+eps, r1..rM) (the same system; float64 accumulation inside).  Orders: forward M <= 2559, backward M <= 1097
 * (dense solve to 85, the symmetric-Toeplitz inverse above); DSA_ERR_UNSUPPORTED beyond (INTEGRATION.md, the ceilings). */
int dsa_levdur_fwd(const void* r, int64_t F, int32_t M, double eps, int32_t dtype, void* out,
                   void* stream);
int dsa_levdur_bwd(const void* gout, const void* r, const void* out, int64_t F, int32_t M, double eps,
                   int32_t dtype, void* gr, void* stream);

/* ------------------------------------------------------------------ a13  LPC
 * LinearPredictiveCodingAnalysis._forward, lpc.py:137-139 = levdur(acorr(x)); x:(F,L) frames. */
int dsa_lpc_fwd(const void* x, int64_t F, int32_t L, int32_t M, double eps, int32_t dtype, void* scratch,
                void* out, void* stream);
int dsa_lpc_bwd(const void* gout, const void* x, const void* out, int64_t F, int32_t L, int32_t M,
                double eps, int32_t dtype, void* gx, void* stream);
/* Fused LPC branch of the README (README.md:198-201): LPC(Window(Frame(x))) in one kernel.
 * x:(B,T), w:(L) or NULL (a window of ones) -> out:(B,N,M+1).  scratch: see Conventions (the tuned kernel for
 * float32 / lpc_order 24 hands out work items through a counter: the first word, which the kernel leaves zeroed).  pad_mode may carry
 * DSA_LPC_SCRATCH_IS_CLEAN: the caller guarantees that the scratch is zero on entry and used by one call at a time (a buffer per
 * stream that only calls with this flag ever touch) -- the library then skips its fill launch, as DSA_ALGO_SCRATCH_IS_CLEAN does. */
#define DSA_LPC_SCRATCH_IS_CLEAN 0x100
int dsa_frame_window_lpc_fwd(const void* x, int64_t B, int64_t T, int32_t L, int32_t P,
                             const void* w, int32_t center, int32_t pad_mode, int32_t M, double eps,
                             int32_t dtype, void* scratch, void* out, void* stream);
/* pad_mode may also carry DSA_LPC_EXACT_LAGSUMS: the tuned float32 kernel then forms its lag sums as exact float64 sums on the
 * vector unit (the kernel of rounds 1-3; ~2.7 x the launch time) instead of 3-term binary16 splits on the matrix pipe (~1e-7 r[0]
 * from the exact sums: what the reference's own float32 FFT route has).  For near-singular frames (a sinusoid plus tiny noise, small
 * eps) whose Toeplitz system amplifies that error.  (The environment variable DSA_LPC_LAGSUMS=f64 still selects it process-wide.) */
#define DSA_LPC_EXACT_LAGSUMS 0x200
/* Its backward in ONE launch -- the adjoint of frame.py:120-141, window.py:185-193, acorr.py:110-120 and levdur.py:113-127
 * composed (README.md:198-201 with a gradient): gout:(B,N,M+1), x:(B,T), w:(L) or NULL -> gx:(B,T), every element written; no
 * (B N, L) tensor in memory either way.  Covers float32, lpc_order 24, 25 <= frame_length <= 512, constant padding and the
 * (frame_length, frame_period) pairs whose overlap fits a wave's LDS stretch; anything else returns DSA_ERR_UNSUPPORTED and the
 * caller composes dsa_lpc_bwd / dsa_window_bwd / dsa_frame_bwd.  A fixed (non-learnable) window: no window gradient. */
int dsa_frame_window_lpc_bwd(const void* gout, const void* x, int64_t B, int64_t T, int32_t L, int32_t P,
                             const void* w, int32_t center, int32_t pad_mode, int32_t M, double eps,
                             int32_t dtype, void* gx, void* stream);

/* ------------------------------------------------------------------ a14  LPC <-> PARCOR and the LPC stability check (0.2.7)
 * Rows are (F, M+1) = [K, c_1 .. c_M]; K is carried, never part of a recursion.  One launch each, float32 and float64 (the
 * recursions run in float64 either way), int64 indexing, no allocation, no host synchronisation; F = 0 is a no-op before any pointer
 * is looked at.  A row's bits depend on (M, dtype) and the row alone, not on F or on its position.  One frame per lane with the
 * recursion unrolled in registers for M <= DSA_PARCOR_MAX_ORDER, one wave per frame with the row in LDS up to
 * DSA_PARCOR_ROW_MAX_ORDER; a larger M is DSA_ERR_INVALID_ARGUMENT.
 *   dsa_lpc2par_fwd   LinearPredictiveCoefficientsToParcorCoefficients._forward, lpc2par.py:103-120: a -> k by the step-down
 *                     recursion on gamma a_1 .. gamma a_M (a^(m-1)_j = (a^(m)_j - k_m a^(m)_{m-j}) / (1 - k_m^2), k_m = a^(m)_m).
 *   dsa_lpc2par_bwd   its adjoint from the OUTPUT k alone (the intermediates are regenerated by stepping up): gk -> ga.
 *   dsa_par2lpc_fwd   ParcorCoefficientsToLinearPredictiveCoefficients._forward, par2lpc.py:101-107: k -> a by the step-up recursion
 *                     (a^(m)_j = a^(m-1)_j + k_m a^(m-1)_{m-j}), the WHOLE row -- K included -- divided by gamma (par2lpc.py:102).
 *   dsa_par2lpc_bwd   its adjoint from the input k: ga -> gk.  Each a^(m-1) is recomputed by stepping up from k, never by stepping
 *                     down from the output: the gradient is finite at |k_m| = 1.
 *   dsa_lpccheck_fwd  LinearPredictiveCoefficientsStabilityCheck._forward, lpccheck.py:104-121: step-down (gamma 1), the PARCOR
 *                     rounded to the dtype, k_1 .. k_M clipped to +-bound (bound rounded to the dtype, as torch.clip does with a
 *                     Python scalar), step-up -> out.  k:(F, M+1) or NULL receives the UNCLIPPED PARCOR for the backward.
 *                     unstable: one int32 or NULL, zeroed by the caller, set to 1 (an ordinary vector store) when any |k_m| >= 1.
 *   dsa_lpccheck_bwd  gout and the forward's k -> ga: the step-up adjoint on the clipped k, torch.clip's mask (1 inside and on the
 *                     bound), the step-down adjoint on the unclipped k. */
#define DSA_PARCOR_MAX_ORDER 32
#define DSA_PARCOR_ROW_MAX_ORDER 1023
int dsa_lpc2par_fwd(const void* a, int64_t F, int32_t M, double gamma, int32_t dtype, void* k, void* stream);
int dsa_lpc2par_bwd(const void* gk, const void* k, int64_t F, int32_t M, double gamma, int32_t dtype, void* ga, void* stream);
int dsa_par2lpc_fwd(const void* k, int64_t F, int32_t M, double gamma, int32_t dtype, void* a, void* stream);
int dsa_par2lpc_bwd(const void* ga, const void* k, int64_t F, int32_t M, double gamma, int32_t dtype, void* gk, void* stream);
int dsa_lpccheck_fwd(const void* a, int64_t F, int32_t M, double bound, int32_t dtype, void* out, void* k, int32_t* unstable,
                     void* stream);
int dsa_lpccheck_bwd(const void* gout, const void* k, int64_t F, int32_t M, double bound, int32_t dtype, void* ga, void* stream);

/* ------------------------------------------------------------------ a15  line spectral pairs: lpc2lsp, lsp2lpc, lspcheck (0.2.8)
 * Rows are (F, M+1) = [K, c_1 .. c_M]; one launch each, float32 and float64 with all arithmetic in float64 and one rounding at the
 * store, int64 indexing, no allocation, no host synchronisation; F = 0 is a no-op before any pointer is looked at.  M < 0 or
 * M > DSA_LSP_MAX_ORDER is DSA_ERR_INVALID_ARGUMENT.  A row's bits depend on (M, dtype, options) and the row alone, not on F or on its
 * position.  `unit` is the angle in radians of one unit of the LSP format (radian 1, cycle 2 pi, khz 2000 pi / sample_rate,
 * hz 2 pi / sample_rate): lpc2lsp divides by it, lsp2lpc multiplies.  log_gain is a flag.
 *   dsa_lpc2lsp_fwd   LinearPredictiveCoefficientsToLineSpectralPairs._forward, lpc2lsp.py:169-197, which deflates the sum and
 *                     difference polynomials (lpc2lsp.py:177-187) and takes the angles of the eigenvalues of their companion
 *                     matrices (lpc2lsp.py:188-192).  Here: the two deflated polynomials as Chebyshev series in cos w, their roots
 *                     bracketed by sign changes on a grid of pi / 64 (halved up to 6 times while fewer than M brackets are found)
 *                     and refined by a fixed number of bisection and Newton steps; one wave per frame.  No eigen-solver.
 *                     A row whose M roots cannot be found or do not interlace (a predictor that is not minimum phase, NaN input)
 *                     gets NaN in w_1 .. w_M, K carried -- a departure: the reference returns the angles of off-circle roots.
 *                     failed: one int32 or NULL, zeroed by the caller, set to 1 (an ordinary vector store) when there is such a row.
 *   dsa_lpc2lsp_bwd   gw, the input a and the OUTPUT w -> ga, by the implicit function theorem on the root's own polynomial; no root
 *                     finder.  A NaN row of w gives NaN in ga_1 .. ga_M.
 *   dsa_lsp2lpc_fwd   LineSpectralPairsToLinearPredictiveCoefficients._forward, lsp2lpc.py:171-195, which multiplies the complex
 *                     roots e^{+-jw} (lsp2lpc.py:180-188) and applies the trivial factors (lsp2lpc.py:148-153, 189-191).  Here: the
 *                     product of the REAL sections 1 - 2 cos w_i z^-1 + z^-2 over the odd- and over the even-indexed LSPs, the same
 *                     trivial factors, a = (p + q) / 2.  The kernel never produces a complex number and never refuses an order
 *                     <= DSA_LSP_MAX_ORDER (the reference raises in float32 from M = 16 on, and in float64 at M = 63).
 *   dsa_lsp2lpc_bwd   ga and the input w -> gw: each section divided out of its product again, O(M^2) per frame, no workspace.
 *   dsa_lspcheck_fwd  LineSpectralPairsStabilityCheck._forward, lspcheck.py:115-145: n_iter Gauss-Seidel sweeps over the pairs
 *                     (lspcheck.py:133-138), each followed by the clip to [min_distance, pi - min_distance] (lspcheck.py:139; the
 *                     bounds rounded to the dtype, as torch.clip does with a Python scalar).  A row stops sweeping when ITS distances
 *                     are all >= min_distance - 1e-16 -- a departure: the reference's break (lspcheck.py:140-142) is batch-wide.
 *                     unstable: one int32 or NULL, zeroed by the caller, set to 1 (an ordinary vector store) by the test of
 *                     lspcheck.py:121, which looks at the whole row, K included.
 *   dsa_lspcheck_bwd  gout and the input w -> gw: the forward replayed to regenerate the masks of each sweep, the piecewise-linear
 *                     adjoint applied in reverse (both clips pass the gradient on their bound); n_iter = 0 is the identity. */
#define DSA_LSP_MAX_ORDER 64
int dsa_lpc2lsp_fwd(const void* a, int64_t F, int32_t M, int32_t log_gain, double unit, int32_t dtype, void* w, int32_t* failed,
                    void* stream);
int dsa_lpc2lsp_bwd(const void* gw, const void* a, const void* w, int64_t F, int32_t M, int32_t log_gain, double unit, int32_t dtype,
                    void* ga, void* stream);
int dsa_lsp2lpc_fwd(const void* w, int64_t F, int32_t M, int32_t log_gain, double unit, int32_t dtype, void* a, void* stream);
int dsa_lsp2lpc_bwd(const void* ga, const void* w, int64_t F, int32_t M, int32_t log_gain, double unit, int32_t dtype, void* gw,
                    void* stream);
int dsa_lspcheck_fwd(const void* w, int64_t F, int32_t M, double min_distance, int32_t n_iter, int32_t dtype, void* out,
                     int32_t* unstable, void* stream);
int dsa_lspcheck_bwd(const void* gout, const void* w, int64_t F, int32_t M, double min_distance, int32_t n_iter, int32_t dtype,
                     void* gw, void* stream);

/* ------------------------------------------------------------------ a16  the MLSA filter's stability check: mlsacheck (0.2.9)
 * MLSADigitalFilterStabilityCheck._forward, mlsacheck.py:181-230.  Rows are (F, M+1) mel-cepstra; one launch each, float32 and float64
 * with all arithmetic in float64 and one rounding at the store, int64 indexing, no allocation, no workspace, no host synchronisation;
 * F = 0 is a no-op before any pointer is looked at.  DSA_ERR_INVALID_ARGUMENT: F < 0 or M < 0, a mode that is none of
 * DSA_MLSACHECK_*, a dtype that is none of DSA_F32 / DSA_F64, in the FFT modes n_fft <= 0 or 2 (n_fft / 2) < M + 1, frames without
 * pointers.  A row's bits depend on (M, dtype, options) and the row alone, not on F or on its position.
 * With gain = sum_m mc_m (-alpha)^m and c = mc except c_0 = mc_0 - gain (mlsacheck.py:191, 198):
 *   DSA_MLSACHECK_FAST   a = max(sum_m c_m, 1e-16), s = min(1, threshold / a), out = s c, out_0 += gain (fast=True; n_fft is not looked at).
 *   DSA_MLSACHECK_SCALE  C_k = sum_m c_m e^{-j 2 pi k m / n_fft}, k < K = n_fft / 2 + 1; a = max(max_k |C_k|, 1e-16), one s = min(1, threshold / a).
 *   DSA_MLSACHECK_CLIP   s_k = min(1, threshold / |C_k|) per bin (|C_k| = 0: 1).
 *   In both FFT modes out_m = (1 / N') sum_k w_k Re(s_k C_k e^{+j 2 pi k m / N'}), m <= M, with N' = 2 (K - 1) -- torch's default irfft
 *   length, n_fft only when that is even -- and w = 2 except w_0 = w_{K-1} = 1, whose imaginary parts are ignored; out_0 += gain.  No FFT
 *   is run: both transforms are (M + 1) x K sums.
 * unstable: one int32 or NULL, zeroed by the caller, set to 1 (an ordinary vector store) when threshold < a in any frame.
 * Two departures from the reference.  (1) Where the two transforms invert each other -- fast mode and every even n_fft -- a frame that
 * nothing clips (a <= threshold) is returned with the INPUT'S BITS and its gradient is the cotangent's bits; the reference re-rounds
 * c_0 through (c_0 - gain) * 1 + gain and the rest through its FFT pair.  (For odd n_fft the reference's irfft(rfft(c)) has another
 * length than it was made with and is another vector than c; such a frame goes through both transforms here as it does there.)
 * (2) The reference returns a tensor of the wrong width when 2 (n_fft / 2) < M + 1 (24 columns for M = 24, n_fft = 25); here that is
 * an invalid argument, and the module raises ValueError at _precompute.
 *   dsa_mlsacheck      mc -> out.
 *   dsa_mlsacheck_vjp  gout and the INPUT mc -> gmc, the exact derivative of the piecewise-smooth forward, everything recomputed from
 *                      mc: through s and the plain sum (fast), through s and the one bin that attains the maximum (scale; among equal
 *                      bins the lowest), through every clipped bin's threshold / |C_k| and the adjoints of the two transforms (clip).  A
 *                      clip that is exactly on its bound passes the gradient, as torch.clip does.
 * float32 with M <= 63 and n_fft = 256 (or fast mode) runs the tuned kernels (one wave per frame, the bins over the lanes, the maximum a
 * wave reduction, the complex exponentials by rotation); everything else the generic ones (one wave per frame, the row and the bins in
 * LDS: DSA_ERR_UNSUPPORTED when 24 (M + 1) + 16 K bytes exceed 144 KiB). */
enum { DSA_MLSACHECK_FAST = 0, DSA_MLSACHECK_SCALE = 1, DSA_MLSACHECK_CLIP = 2 };
int dsa_mlsacheck(const void* mc, int64_t F, int32_t M, double alpha, double threshold, int32_t mode, int32_t n_fft, int32_t dtype,
                  void* out, int32_t* unstable, void* stream);
int dsa_mlsacheck_vjp(const void* gout, const void* mc, int64_t F, int32_t M, double alpha, double threshold, int32_t mode, int32_t n_fft,
                      int32_t dtype, void* gmc, void* stream);

/* ------------------------------------------------------------------ a17  excitation generation: excite (0.3.0)
 * ExcitationGeneration._forward, excite.py:222-310.  p:(B, N) pitch in samples, 0 = unvoiced -> out:(B, N P), the VOICED part of the
 * excitation and zeros in every unvoiced sample (the host layer fills those: modules/excite.py); one launch, float32 and float64,
 * int64 indexing, no allocation, no workspace, no host synchronisation; B = 0 or N = 0 is a no-op before any pointer is looked at.
 * DSA_ERR_INVALID_ARGUMENT: B < 0, N < 0, P < 1 or P > 2^20, B N P beyond int64, a type that is none of DSA_EXCITE_*, a dtype that is
 * none of DSA_F32 / DSA_F64, frames without pointers.
 * Per voiced frame n (p_n != 0) and sample j < P, everything in the data's dtype except the sum:
 *   target  b = p_{n+1}, or p_n when frame n + 1 is unvoiced or n is the last frame     (excite.py:236-239 and the replicate pad of
 *           linear_intpl.py:99)
 *   pitch   a + (j / P) (b - a), a = p_n                                                 (linear_intpl.py:100-105)
 *   q       1 / pitch, correctly rounded                                                 (excite.py:262)
 *   phase   the FLOAT64 sum of q from the first sample of the voiced run through this one, rounded to the dtype, plus the shift
 *           (excite.py:263-265, 282, 294)
 * and then the shape, bipolar != 0 selecting its bipolar form:
 *   DSA_EXCITE_PULSE           sqrt(pitch) where ceil(phase) exceeds ceil of the phase of the sample before by >= 1 (the shift alone at
 *                              the start of an utterance and after an unvoiced sample); bipolar: negated where ceil(phase / 2) does not
 *                              rise as well                                              (excite.py:28-44)
 *   DSA_EXCITE_HARMONIC_PULSE  the Dirichlet kernel of floor(pitch / 2) harmonics on the phase of the sample BEFORE, its singular branch
 *                              at |2 sin(theta / 2)| < 1e-6, times sqrt(2 / max(harmonics, 1))   (excite.py:47-77)
 *   DSA_EXCITE_SINUSOIDAL, _SAWTOOTH, _INVERTED_SAWTOOTH, _TRIANGLE, _SQUARE              (excite.py:80-114)
 * shift: B values of the dtype (the initial phase / 2 pi per utterance: init_phase "random"), or NULL: then init_shift for every
 * utterance.
 * For float32 data the float64 sums are exact, so the result does not depend on how the sum is split over lanes, waves and chunks: an
 * utterance's bits depend on (P, options, shift) and its own N values, not on B, its row or where a voiced run lies in it.
 * Four departures from the reference.  (1) p is NOT modified (the reference overwrites the unvoiced frame behind every voiced run in
 * place).  (2) The interpolated pitch is a + w (b - a) as in the library's filters, which differs from F.interpolate in the last place
 * on some samples.  (3) Negative pitch values and values in (0, 1) are outside the contract (the reference's masks disagree with each
 * other there).  (4) The host layer returns an ordinary tensor without a gradient, where the reference returns an inference tensor.
 * One workgroup per utterance (a grid-stride loop beyond 65 536), 256 frames at a time: per-frame sums, a segmented scan over them, then
 * lane = sample with a segmented wave scan inside the frame.  A single long utterance is correct and runs on one compute unit. */
enum { DSA_EXCITE_PULSE = 0, DSA_EXCITE_HARMONIC_PULSE = 1, DSA_EXCITE_SINUSOIDAL = 2, DSA_EXCITE_SAWTOOTH = 3,
       DSA_EXCITE_INVERTED_SAWTOOTH = 4, DSA_EXCITE_TRIANGLE = 5, DSA_EXCITE_SQUARE = 6 };
int dsa_excite(const void* p, int64_t B, int64_t N, int32_t P, int32_t type, int32_t bipolar, double init_shift, const void* shift,
               int32_t dtype, void* out, void* stream);

/* ------------------------------------------------------------------ a18  lapped transforms: mdct, imdct, mdst, imdst (0.3.1)
 * ModifiedDiscreteCosineTransform._forward, mdct.py:166-176, with the basis of ModifiedDiscreteTransform._precompute, mdct.py:253-285;
 * InverseModifiedDiscreteCosineTransform._forward, imdct.py:169-181.  P = L/2, L >= 2 and even.
 *   basis   C[j,k] = z cos(pi/P (j + 1/2 + P/2)(k + 1/2)), sin for DSA_MDCT_SINE; z = sqrt(4/P), sqrt(2/P) for the rectangular window
 *   dsa_mdct_analysis   x:(B,T) -> y:(B,N,P),  y[n,k] = sum_{j<L} w[j] s[t] x[t] C[j,k] at t = (n-1)P + j, x = 0 outside [0, T);
 *                       1 <= T <= N P (the host layer passes N = (T + P - 1) / P + 1, the frames of the reference's padded signal)
 *   dsa_mdct_synthesis  y:(B,N,P) -> x:(B,T),  x[t] = s[t] sum_n w[j] sum_k y[n,k] C[j,k] at j = t + P - nP in [0, L): the two frames
 *                       t / P and t / P + 1, the older one first; 0 <= T <= N P
 *   scale   DSA_MDCT_SCALE_NONE: s = 1.  DSA_MDCT_SCALE_OVERLAP: s[t] = 1/2 for t < (N-1)P, else 1 -- Unframe's division by the number
 *           of frames over a sample (imdct.py:178; its divisor c + 1e-16 rounds to exactly 2 or 1 in both dtypes), applied while the
 *           synthesis stores and while the analysis loads.
 * Each entry is the other's adjoint: d/dx of analysis(SCALE_NONE) is synthesis(SCALE_NONE) at the same T and N, d/dy of
 * synthesis(scale) is analysis(scale) of the cotangent -- two kernel families serve all eight directions of the four operators.
 * Tables, built by the host layer in float64 and cast to the dtype (device pointers, read-only):
 *   w        (L)  Window(L, norm="none", symmetric=True)
 *   basis    (L, P) for the analysis, basis_t (P, L), its transpose, for the synthesis: C above with z folded in.  The generic kernels
 *            read it; NULL when the fast kernels are to run.
 *   twiddle  3P/2 values of the dtype: P/2 pairs (cos, -sin)(pi (8n + 1) / (8P)) and P/4 pairs (cos, -sin)(2 pi m / (P/2)).  The fast
 *            kernels read it, with z as a scalar; NULL selects the generic kernels.
 * algo: DSA_ALGO_AUTO runs the fast kernels when dtype is DSA_F32, L is a power of two in DSA_MDCT_FAST_MIN_LENGTH ..
 * DSA_MDCT_FAST_MAX_LENGTH and `twiddle` is given (or `basis` is not); DSA_ALGO_GENERIC never does; DSA_ALGO_TUNED returns
 * DSA_ERR_UNSUPPORTED where they cannot.  dsa_last_kernel(): "mdct_analysis_fast", "mdct_analysis_generic", "mdct_synthesis_fast",
 * "mdct_synthesis_generic".
 * One launch, no allocation, no workspace, no atomics (every output element is written once, by one thread: deterministic), int64
 * indexing; B = 0 or N = 0 (and T = 0 in the synthesis) is a no-op before any pointer is looked at.  DSA_ERR_INVALID_ARGUMENT with
 * a message that names "mdct": L odd or < 2, a negative size, T > N P, T < 1 in the analysis, a transform / scale / dtype / algo that
 * is none of the enumerators, more than 2^31 - 1 tiles, a missing pointer.
 * A frame's bits depend on (L, tables, options) and its own 2P samples (P coefficients), not on B, N, T or its place in them. */
enum { DSA_MDCT_COSINE = 0, DSA_MDCT_SINE = 1 };
enum { DSA_MDCT_SCALE_NONE = 0, DSA_MDCT_SCALE_OVERLAP = 1 };
#define DSA_MDCT_FAST_MIN_LENGTH 16
#define DSA_MDCT_FAST_MAX_LENGTH 4096
int dsa_mdct_analysis(const void* x, int64_t B, int64_t T, int64_t N, int32_t L, const void* w, const void* basis, const void* twiddle,
                      double z, int32_t transform, int32_t scale, int32_t dtype, int32_t algo, void* y, void* stream);
int dsa_mdct_synthesis(const void* y, int64_t B, int64_t N, int32_t L, const void* w, const void* basis_t, const void* twiddle, double z,
                       int32_t transform, int32_t scale, int64_t T, int32_t dtype, int32_t algo, void* x, void* stream);

/* ------------------------------------------------------------------ a19  parameter generation: delta, mlpg, mcpf (0.3.2)
 * The stage between an acoustic model's output and mlsacheck -> excite -> MLSA.  float32 and float64; every sum is taken in float64.
 * No allocation, no atomics, int64 indexing, one launch per entry (dsa_mlpg: two); a result's bits depend on its own column (delta, mlpg) or frame
 * (mcpf), not on the batch around it.  B = 0, T = 0 or D = 0 (mcpf: F = 0) is a no-op before any pointer is looked at.
 * DSA_ERR_INVALID_ARGUMENT with a message that names the operator: a negative size, H or L outside 1 .. 1024, an even L, a dtype or
 * direction that is none of the enumerators, a missing pointer, and what each entry lists below.
 *
 * Delta._forward, delta.py:181-201 (the window of Delta._precompute, delta.py:105-178, from the host: (H, L) of the dtype, L odd,
 * N = (L - 1) / 2):
 *   dsa_delta  x:(B,T,D) -> y:(B,T,H,D)   y[b,t,h,d] = sum_j window[h,j] x[b, clamp(t + j - N, 0, T - 1), d]
 *   dsa_delta_vjp  gy:(B,T,H,D) -> gx:(B,T,D) the adjoint as a gather: row s sums window[h,j] gy[t,h] over the t with
 *                  clamp(t + j - N) = s -- one t inside, up to N + 1 at rows 0 and T - 1, where the replicate padding folds
 *
 * MaximumLikelihoodParameterGeneration._forward, mlpg.py:165-171, with the matrix of _precompute, mlpg.py:126-163, never formed:
 *   W:(T H, T)   W[(t,h), s] = window[h, s - t + N] for 0 <= s - t + N < L, kept where t < N ? th[h] <= t : (t > T - N - 1 ? th[h] < T - t : 1)
 *                (mlpg.py:146-156: the first and last N rows drop a dynamic window whose half-width th[h] does not fit; th[0] = 0)
 *   A = W^T W    symmetric positive definite, banded with half-bandwidth K = 2N = L - 1; A = G G^T, G lower banded
 *   factor:(T, K + 1) of the dtype, from the host in float64: factor[s, i] = G[s, s - K + i] for i < K (0 left of column 0),
 *                factor[s, K] = 1 / G[s, s]
 *   dsa_mlpg, DSA_MLPG_FORWARD   u:(B,T,H,D) -> out:(B,T,D) = A^-1 W^T u: the right-hand side as a gather into out, then forward and
 *                back substitution per column (b, d) in place; `work` is not read (NULL)
 *   dsa_mlpg, DSA_MLPG_ADJOINT   u:(B,T,D), the cotangent -> out:(B,T,H,D) = W A^-1 u: the sweeps into work:(B,T,D) of the dtype,
 *                then W applied to it
 *   th:(H) int32 on the device.  One lane per column; the last K values of the recurrence stay in registers for K <=
 *   DSA_MLPG_MAX_REGISTER_BAND and are read back from the column otherwise.  dsa_last_kernel(): "mlpg_forward_reg", "mlpg_adjoint_reg",
 *   "mlpg_forward_any", "mlpg_adjoint_any".  T < L - 1 is an invalid argument: the reference cannot build its matrix there either
 *   (a shape mismatch at mlpg.py:152).
 *
 * MelCepstrumPostfiltering._forward, mcpf.py:191-209 (freqt.py, c2acr.py:97-101, mc2b.py, b2mc.py), in closed form:
 *   out[j] = w[j] mc[j], w[j] = 1 for j < onset, else scale = 1 + beta;   out[0] += log(e1 / e2) / 2
 *   e = sum_{k < bins} u_k exp(2 s_k), u_k = 1 at k = 0 and k = bins - 1, else 2 (the reference's hfft over bins = ir_length / 2 + 1
 *   values has 2 (bins - 1) points: ir_length - 1 of them for an odd ir_length; the factor 1 / n cancels in the ratio);
 *   s = R mc for e1, s = R (w mc) for e2;   R[k,j] = sum_{m < ir_length} cos(2 pi k m / ir_length) A[m,j], A the freqt matrix of -alpha
 *   table:(bins, M1) = R and table_t:(M1, bins) = R^T, FLOAT64 for either dtype, from the host
 *   dsa_mcpf  mc:(F,M1) -> out:(F,M1)
 *   dsa_mcpf_vjp  mc, g:(F,M1) -> gmc:(F,M1): the adjoint of the Jacobian at mc; nothing is saved by the forward
 *   One wave per frame, the bins over the lanes.  2 <= bins <= DSA_MCPF_MAX_BINS, onset >= 0 (it may exceed M1), scale finite. */
enum { DSA_MLPG_FORWARD = 0, DSA_MLPG_ADJOINT = 1 };
#define DSA_MLPG_MAX_REGISTER_BAND 8
#define DSA_MCPF_MAX_BINS 2049
int dsa_delta(const void* x, int64_t B, int64_t T, int64_t D, const void* window, int32_t H, int32_t L, int32_t dtype, void* y, void* stream);
int dsa_delta_vjp(const void* gy, int64_t B, int64_t T, int64_t D, const void* window, int32_t H, int32_t L, int32_t dtype, void* gx, void* stream);
int dsa_mlpg(const void* u, int64_t B, int64_t T, int64_t D, const void* window, const void* th, int32_t H, int32_t L, const void* factor,
             int32_t direction, int32_t dtype, void* work, void* out, void* stream);
int dsa_mcpf(const void* mc, int64_t F, int32_t M1, const void* table_t, int32_t bins, double scale, int32_t onset, int32_t dtype, void* out,
                 void* stream);
int dsa_mcpf_vjp(const void* mc, const void* g, int64_t F, int32_t M1, const void* table, const void* table_t, int32_t bins, double scale,
                 int32_t onset, int32_t dtype, void* gmc, void* stream);

/* ------------------------------------------------------------------ a20  dynamic time warping with a soft minimum: dtw (0.3.4)
 * DynamicTimeWarping._forward, dtw.py:301-338, with the core of dtw.py:26-125: the reference's T1 T2 Python iterations as one launch.
 * x:(B,T1,D), y:(B,T2,D) of the dtype; lengths:(B,2) int64 on the device, or NULL for (T1, T2) everywhere.  float32 and float64, int64
 * indexing, no allocation, no atomics, no host synchronisation.  A pair's bits depend on (T1, T2, D, options) and its own values, not on
 * B or its place in the batch.  B = 0 is a no-op before any pointer is looked at.
 *   d(i,j)    DSA_DTW_MANHATTAN sum |x - y|; _EUCLIDEAN sqrt(sum (x - y)^2); _SQUARED_EUCLIDEAN that root squared (as the reference);
 *             _SYMMETRIC_KL sum x log(max(x / y, 1e-10)) + sum y log(max(y / x, 1e-10)): formed in the kernel, never stored
 *   steps     of the local path constraint p = 0 .. 6, in the order of dtw.py:255-284; p = 4 and 6 keep a second table R_
 *   R[i,j]    -softness logsumexp(-c_k / softness) over c_k = (a + b) d(i,j) + S[i - a, j - b] of the steps (a, b) whose source is inside
 *             and not +inf; S = R_ for an axis step (a = 0 or b = 0) of p = 4, 6, else R; R_[i,j] the same over the other steps;
 *             R[0,0] = d(0,0), R_[0,0] = +inf
 *   dsa_dtw       distance[b] = R[len1 - 1, len2 - 1] / (len1 + len2), +inf when the end is unreachable; NaN for lengths outside
 *                 1 .. T1, 1 .. T2.  R, R2: the tables, T1 T2 values of the dtype per pair each (R2 only for p = 4, 6; else NULL), laid
 *                 out by anti-diagonal; cells outside the pair's lengths are not written.  R = NULL: nothing but the distance is stored.
 *   dsa_dtw_vjp   dtw.py's autograd in closed form: gx:(B,T1,D), gy:(B,T2,D), every element written, for the cotangent gdistance:(B) and
 *                 the tables of dsa_dtw.  Zero for a pair with an unreachable end or invalid lengths.  d/dx of |.| is sign with
 *                 sign(0) = 0, of the Euclidean distance 0 where d = 0; a clipped quotient passes no derivative.
 *   dsa_dtw_path  indices:(B, T1 + T2 - 1, 2) int64 and count:(B) int32: the pair's Viterbi path (dtw.py:106-123; the hard argmin of each
 *                 visited cell recomputed from the tables, ties to the first step) is rows [T1 + T2 - 1 - count, T1 + T2 - 1) in forward
 *                 order, the rows before them are not written; count = 1 for an unreachable end, 0 for invalid lengths.
 * Workspace: the caller's R (and R2), T1 T2 elements per pair each, between dsa_dtw and the other two; the library owns no device memory.
 * One workgroup per pair, x_b in LDS: T1 <= 64 runs in one wave, rows over the lanes, neighbours by lane exchange, no barrier; longer x
 * runs rows strided over up to 1024 threads with the last three diagonals in LDS and one barrier per diagonal.  dsa_last_kernel():
 * "dtw_wave_f32", "dtw_block_f32", "dtw_vjp_wave_f32", "dtw_vjp_block_f32", "dtw_path_f32" and the same with f64.
 * DSA_ERR_INVALID_ARGUMENT with a message that names "dtw": a negative size, T1 or T2 = 0, sizes beyond int64, a metric / p / dtype
 * that is none of the above, softness <= 0, a missing pointer, and T1 (D + 12) sizeof(dtype) > DSA_DTW_MAX_LDS_BYTES: one pair's x and
 * the resident diagonals have to fit one compute unit's LDS (float32 at D = 25: T1 <= 1107). */
enum { DSA_DTW_MANHATTAN = 0, DSA_DTW_EUCLIDEAN = 1, DSA_DTW_SQUARED_EUCLIDEAN = 2, DSA_DTW_SYMMETRIC_KL = 3 };
#define DSA_DTW_MAX_LDS_BYTES 163840
int dsa_dtw(const void* x, const void* y, const void* lengths, int64_t B, int64_t T1, int64_t T2, int64_t D, int32_t metric, int32_t p,
            double softness, int32_t dtype, void* R, void* R2, void* distance, void* stream);
int dsa_dtw_vjp(const void* x, const void* y, const void* lengths, const void* R, const void* R2, const void* gdistance, int64_t B, int64_t T1,
                int64_t T2, int64_t D, int32_t metric, int32_t p, double softness, int32_t dtype, void* gx, void* gy, void* stream);
int dsa_dtw_path(const void* x, const void* y, const void* lengths, const void* R, const void* R2, int64_t B, int64_t T1, int64_t T2, int64_t D,
                 int32_t metric, int32_t p, int32_t dtype, void* indices, void* count, void* stream);

/* ------------------------------------------------------------------ a21  Gaussian mixture models: gmm (0.3.5)
 * GaussianMixtureModeling.forward / _e_step / transform, gmm.py:241-486.  K components of dimension L; w:(K), mu:(K,L), sigma:(K,L,L),
 * x:(T,L') of the dtype, L' <= L the leading block an entry works on (L' = L while training; L' = N + 1 in transform: the pointers stay,
 * the leading dimension L tells the rows apart, nothing is copied).  diag != 0 is the route of var_type "diag" with one block: only the
 * diagonal of sigma is read and written.  float32 and float64, int64 indexing, no floating-point atomics: every sum has one fixed
 * order, two runs give the same bits.  The library owns no device memory; the caller passes every workspace.
 *   dsa_gmm_prepare   prec:(K,L',L') the inverse W_k of the Cholesky factor of sigma_k's leading block (zero above the diagonal), or on the
 *                     diagonal route prec:(K,L') the reciprocal variances; cst:(K) c_k = log w_k - (L' log 2 pi + log det) / 2; failed:(K)
 *                     int32, 1 where a pivot was not positive (then W_k = 0 and c_k = -inf), else 0.  The diagonal route never fails: a
 *                     variance that is not positive gives the reference's inf / NaN.
 *   dsa_gmm_estep     posterior:(T,K) exp(numer - logsumexp_k numer), numer[t,k] = c_k - |W_k (x_t - mu_k)|^2 / 2 (diagonal route: the
 *                     weighted squares); loglik:(T) the log-sum-exp, maximum first as torch.logsumexp; partial: ceil(T / rows) float64
 *                     per-workgroup sums, rows = DSA_GMM_TILE_BYTES / sizeof(dtype) vectors per workgroup; total (1 of the dtype, or NULL)
 *                     their sum; readback (2 float64, or NULL): the total and the first k + 1 with failed[k], 0 when none -- what the
 *                     host reads once per iteration.  Both NULL: no second launch.
 *   dsa_gmm_accum     the weighted moment sums into workspace (dsa_gmm_accum_workspace_bytes: S K (L + 1)^2 elements, on the diagonal
 *                     route S K (2 L + 1); S <= 64 segments of T of at least 256 vectors, and S > 1 only while S times the waves of one
 *                     segment stay below 8192: at most 8192 32 x 32 tiles of the dtype, 64 MiB; 15 MiB at K = 64, L = 50, float32).  Segment s, component k: the lower triangle, by 32 x 32
 *                     tiles, of sum_t p[t,k] a a^T, a = [x_t, 1] -- row L is px, the corner z; diagonal route: px (L), z, pxx (L).
 *   dsa_gmm_update    gmm.py:303-378 from the partial sums, added in segment order: w (z / T or (z + alpha ubm_w) / (T + alpha), floored,
 *                     renormalised a w + b), mu, sigma (MAP when alpha != 0, with nan_to_num on the data term; times mask:(L,L); the
 *                     diagonal floored at var_floor), written in place.  readback != NULL and readback[1] != 0: nothing is written.
 *   dsa_gmm_regress   M:(K, L - Lx, Lx) = sigma[:, Lx:, :Lx] inverse(sigma[:, :Lx, :Lx]) by Gauss-Jordan elimination with partial
 *                     pivoting; a singular block gives inf / NaN, not an error.
 *   dsa_gmm_transform indices:(T) int64 the first largest posterior; y:(T, L - Lx) = mu[k, Lx:] + M_k (x_t - mu[k, :Lx]), or y = NULL.
 * dsa_last_kernel(): "gmm_prepare_full_f32", "gmm_prepare_diag_f32", "gmm_estep_*", "gmm_accum_*", "gmm_update_*" likewise,
 * "gmm_regress_f32", "gmm_transform_f32", and the same with f64.
 * DSA_ERR_INVALID_ARGUMENT with a message that names "gmm": a size below 1, L' > L, sizes beyond int64, an unknown dtype, a missing
 * pointer, options outside their ranges, and 2 DSA_GMM_TILE_BYTES (L + 1) + L (L + 1) sizeof(dtype) + 64 > DSA_GMM_MAX_LDS_BYTES: the
 * E-step's workgroup holds its vectors, their differences, one component's matrix and mean and its reduction scratch in LDS
 * (float32: L <= 69, float64: L <= 63; L is L' for prepare, estep, regress and transform). */
#define DSA_GMM_MAX_LDS_BYTES 163840
#define DSA_GMM_TILE_BYTES 1024
int dsa_gmm_prepare(const void* w, const void* sigma, int64_t K, int64_t L, int64_t Lp, int32_t diag, int32_t dtype, void* prec, void* cst,
                    void* failed, void* stream);
int dsa_gmm_estep(const void* x, const void* mu, const void* prec, const void* cst, const void* failed, int64_t T, int64_t K, int64_t L,
                  int64_t Lp, int32_t diag, int32_t dtype, void* posterior, void* loglik, void* partial, void* total, void* readback,
                  void* stream);
int64_t dsa_gmm_accum_workspace_bytes(int64_t T, int64_t K, int64_t L, int32_t diag, int32_t dtype);
int dsa_gmm_accum(const void* x, const void* posterior, int64_t T, int64_t K, int64_t L, int32_t diag, int32_t dtype, void* workspace,
                  void* stream);
int dsa_gmm_update(const void* workspace, const void* readback, const void* ubm_w, const void* ubm_mu, const void* ubm_sigma, const void* mask,
                   int64_t T, int64_t K, int64_t L, int32_t diag, double alpha, double weight_floor, double var_floor, int32_t dtype, void* w,
                   void* mu, void* sigma, void* stream);
int dsa_gmm_regress(const void* sigma, int64_t K, int64_t L, int64_t Lx, int32_t dtype, void* M, void* stream);
int dsa_gmm_transform(const void* x, const void* posterior, const void* mu, const void* M, int64_t T, int64_t K, int64_t L, int64_t Lx,
                      int32_t dtype, void* indices, void* y, void* stream);

/* ------------------------------------------------------------------ a22  Yingram, the pitch feature of YIN on a semitone grid (0.3.6)
 * Yingram._forward, yingram.py:167-194.  x:(F,L) frames of the dtype, lag_max = K with 1 <= K < L; the tables of Yingram._precompute,
 * yingram.py:127-164, as the module holds them: lags:(M) of the dtype, non-increasing, lags_floor, lags_ceil:(M) int64 with
 * 0 <= floor <= ceil <= K - 1 (the kernels clamp what they index with).  Per frame
 *   d[tau]  = sum_{j < L - tau} (x[j] - x[j + tau])^2, tau = 1 .. K - 1;   d'[tau] = tau d[tau] / (sum_{k <= tau} d[k] + 1e-7), d'[0] = 1;
 *   y[m]    = d'[floor_m] + (lags_m - floor_m) (d'[ceil_m] - d'[floor_m]):  where ceil_m = floor_m (an integral lag) y[m] = d'[floor_m].
 * float32 and float64, int64 indexing, no allocation, no atomics, no host synchronisation; the scans run in float64.  A frame's bits
 * depend on (L, K, the tables, the route) and its own values, not on F or its place in the batch.  F = 0 or M = 0 is a no-op before any
 * pointer is looked at.
 *   dsa_yingram        y:(F,M).  One launch; no (F, K) intermediate in memory.
 *   dsa_yingram_vjp        gx:(F,L), every element written, for the cotangent gy:(F,M): the adjoint of the three steps, d recomputed.
 *   dsa_frame_yingram  y:(B,N,M) from the waveform x:(B,T): Frame(L, P, center) with constant padding and zmean = False
 *                          (frame.py:120-141) read on the fly, then the same arithmetic as dsa_yingram, bit for bit.
 * algo: DSA_ALGO_GENERIC the direct route (the lag sums as written, each square added in float64; up to four short frames per
 * workgroup), DSA_ALGO_TUNED the fft route (d from float64 prefix sums of x^2 and the autocorrelation through the LDS transform of
 * 2 H >= L + K points, H a power of two, real input packed as H complex points; needs twiddle: (cos, -sin)(2 pi m / 2H), m < H, of the
 * dtype, else NULL), DSA_ALGO_AUTO the fft route from L = DSA_YINGRAM_FFT_MIN_FRAME_LENGTH on.  dsa_last_kernel():
 * "yingram_direct_f32", "yingram_fft_f32", "yingram_vjp_direct_f32", "yingram_vjp_fft_f32", "frame_yingram_direct_f32",
 * "frame_yingram_fft_f32" and the same with f64.
 * DSA_ERR_INVALID_ARGUMENT with a message that names "yingram": a negative size, L < 2, K outside 1 .. L - 1, F beyond int32, an unknown
 * dtype or algo, a missing pointer, and DSA_YINGRAM_LDS_BYTES(H, L, sizeof(dtype)) > DSA_YINGRAM_MAX_LDS_BYTES at the H of the longest
 * lag range, 2 H the power of two from 2 L - 1 on: the fft route holds the transform's two arrays, one more of H + 1 values, L + 1
 * float64 prefix sums and its scan's exchange in LDS (float32: L <= 8174, float64: L <= 4096; the same ceiling on both routes). */
#define DSA_YINGRAM_MAX_LDS_BYTES 163840
#define DSA_YINGRAM_LDS_BYTES(H, L, size) ((3 * (H) + 1) * (size) + 8 * ((L) + 1) + 128)
#define DSA_YINGRAM_FFT_MIN_FRAME_LENGTH 76
int dsa_yingram(const void* x, int64_t F, int32_t L, int32_t lag_max, const void* lags, const void* lags_floor, const void* lags_ceil,
                    int32_t M, const void* twiddle, int32_t algo, int32_t dtype, void* y, void* stream);
int dsa_yingram_vjp(const void* gy, const void* x, int64_t F, int32_t L, int32_t lag_max, const void* lags, const void* lags_floor,
                    const void* lags_ceil, int32_t M, const void* twiddle, int32_t algo, int32_t dtype, void* gx, void* stream);
int dsa_frame_yingram(const void* x, int64_t B, int64_t T, int32_t L, int32_t P, int32_t center, int32_t lag_max, const void* lags,
                          const void* lags_floor, const void* lags_ceil, int32_t M, const void* twiddle, int32_t algo, int32_t dtype, void* y,
                          void* stream);

/* ------------------------------------------------------------------ a23  Vector quantisation and codebook design: vq (0.3.7)
 * VectorQuantization.forward, vq.py:110-125 (nearest codeword, there inside the package vector_quantize_pytorch); InverseVectorQuantization
 * .forward, ivq.py:63-67; one iteration of LindeBuzoGrayAlgorithm.forward, lbg.py:214-224 (E-step) and lbg.py:264-285 (counts and
 * centroids; there a (B, K) distance matrix, histc and scatter_add_ per DataLoader batch).  x:(T,L) of the dtype (float32 or float64),
 * codebook:(K,L) float32 whatever the dtype, indices:(T) int64.  int64 indexing, no allocation, no host synchronisation, no
 * floating-point atomics: every sum has one fixed order, two runs give the same bits.  The library owns no device memory.  T = 0 (and
 * n = 0 of dsa_vq_vjp) is a no-op before any pointer is looked at.
 *   dsa_vq_search   indices[t] = the first k that minimises sum_j (x[t,j] - codebook[k,j])^2, the differences and the sums formed in
 *                   float64 from the values as stored, j ascending: the assignment of exact arithmetic apart from ties closer than
 *                   float64 rounding.  xq:(T,L) of the dtype = codebook[indices], or NULL.  partial: ceil(T / rows) float64, the
 *                   per-workgroup sums of the minimal distances, rows = DSA_VQ_TILE_BYTES / sizeof(dtype) vectors per workgroup (one
 *                   thread per vector, the tile in LDS, the codebook staged through LDS DSA_VQ_CHUNK codewords at a time: K has no
 *                   ceiling).  total (1 of the dtype, or NULL): scale times the sum of the partials, by a second launch of one workgroup.
 *   dsa_vq_accum    per codeword the number and the float64 sum of the vectors assigned to it, into workspace
 *                   (dsa_vq_accum_workspace_bytes: S K L float64 sums, then S K int64 counts; S <= DSA_VQ_MAX_SEGMENTS segments of T of
 *                   at least 256 vectors, as many as fill the chip).  A workgroup takes one segment and as many codewords as fit 64 KiB
 *                   of LDS (16384 / (8 L + 4)); its four waves take every fourth run of 64 vectors each, a lane one column, so every LDS cell
 *                   belongs to one thread.  An index outside 0 .. K - 1 is counted nowhere.
 *   dsa_vq_update   from the workspace (per column the segments s = g, g + 4, ... added in order for g = 0 .. 3, the four runs then in the
 *                   order of g: one fixed order), two launches: n_data:(K) int64; pending:(K,L) float32 = (float)(sum / count) where
 *                   count >= min_data, else 0 (lbg.py:265-285) -- a buffer of the caller's, not the codebook the search read; readback
 *                   (3 float64): the sum of `partial` (n_partial values, may be 0) / T, the number of codewords with count < min_data,
 *                   the first k with the largest count -- what the host reads once per iteration.
 *   dsa_vq_lookup   xq:(T,L) of the dtype = codebook[indices] (ivq.py:65); an index outside 0 .. K - 1 gives a row of NaN.
 *   dsa_vq_vjp      gx[i] = g_xq[i] + g_loss[0] 2 (x[i] - xq[i]) / n, i < n = T L: the straight-through estimator plus the gradient of
 *                   loss = mean((x - xq)^2); g_xq (n of the dtype) or g_loss (1 of the dtype) may be NULL: zero.  One launch.
 * dsa_last_kernel(): "vq_search_f32", "vq_accum_f32", "vq_lookup_f32", "vq_vjp_f32" and the same with f64; "vq_update".
 * DSA_ERR_INVALID_ARGUMENT with a message that names "vq": a negative T, K < 1, L < 1, sizes beyond int64 / int32 launch dimensions,
 * min_data < 1, an unknown dtype, a missing pointer, and L > DSA_VQ_MAX_LENGTH: the accumulation gives a lane of its wave to each
 * column, and the search's tile of vectors (DSA_VQ_TILE_BYTES (L | 1) bytes) shares LDS with the staged codewords. */
#define DSA_VQ_MAX_LENGTH 64
#define DSA_VQ_TILE_BYTES 1024
#define DSA_VQ_CHUNK 64
#define DSA_VQ_MAX_SEGMENTS 256
int dsa_vq_search(const void* x, const void* codebook, int64_t T, int64_t K, int64_t L, int32_t dtype, void* indices, void* xq, void* partial,
                  void* total, double scale, void* stream);
int64_t dsa_vq_accum_workspace_bytes(int64_t T, int64_t K, int64_t L);
int dsa_vq_accum(const void* x, const void* indices, int64_t T, int64_t K, int64_t L, int32_t dtype, void* workspace, void* stream);
int dsa_vq_update(const void* workspace, const void* partial, int64_t n_partial, int64_t T, int64_t K, int64_t L, int64_t min_data,
                  void* n_data, void* pending, void* readback, void* stream);
int dsa_vq_lookup(const void* indices, const void* codebook, int64_t T, int64_t K, int64_t L, int32_t dtype, void* xq, void* stream);
int dsa_vq_vjp(const void* g_xq, const void* g_loss, const void* x, const void* xq, int64_t n, int32_t dtype, void* gx, void* stream);

/* ------------------------------------------------------------------ a24  WORLD synthesis: world_synth (0.3.9)
 * WorldSynthesis.forward, world_synth.py:166-321, with get_minimum_phase_spectrum and interp1 of third_party/world/common.py:73-84, 141-163.
 * f0:(B,N) in Hz, ap, sp:(B,N,D) with D = L / 2 + 1, all of the dtype (float32 or float64); P = frame_period, L = fft_length; the waveform has
 * N P samples per utterance.  int64 indexing, no atomics, no allocation: the same inputs give the same bits every run, and an utterance's
 * bits are those of the utterance run alone.  B = 0, N = 0 or pulses = 0 is a no-op before any pointer is looked at.
 *   dsa_world_synth_pulses       world_synth.py:193-237, one workgroup per utterance: F0 and the voicing flag interpolated to the samples
 *                                (interp1 as it is written: arange(T) / sr, arange(N) (P / sr), diff(y) / diff(x), b = y - m x, m xq + b, the
 *                                segment of searchsorted(right = False) with its padded ends), every product and sum rounded on its own
 *                                in the dtype; the float64 sum of (tau / sr) f0, added in order by one lane (the bits of torch.cumsum:
 *                                the fractional shifts follow the last place of the phase), cast to the dtype, fmod tau, a pulse
 *                                where pi < |the difference of neighbours|.
 *                                counts:(B) int64 is always written.  With irec = frec = NULL nothing else is; with offsets:(B + 1) int64
 *                                (the exclusive prefix sums of counts, which the HOST forms: its one read) the pulses of utterance b go,
 *                                in time order, to rows offsets[b] .. offsets[b + 1] - 1 of irec:(pulses,4) int64 = sample index,
 *                                utterance, floor frame, ceil frame (both clipped to N - 1) and frec:(pulses,3) of the dtype = the
 *                                fractional time shift in seconds, the upper weight frame - floor, the voiced flag (0 or 1).
 *   dsa_world_synth_responses    world_synth.py:233-301, one workgroup per pulse: response:(pulses,L) from the two rows of sp and ap
 *                                (interpolated, clipped at 1e-6 / 1 - 1e-6), noise:(pulses,L) standard normal numbers, dc_remover:(L) as the
 *                                module holds it and twiddle:(L,2) = (cos, -sin)(2 pi m / L).  noise_size of a pulse is the distance to the
 *                                next pulse OF ITS UTTERANCE, 0 for the last one (the reference takes diff over the flattened batch: the
 *                                last pulse of an utterance that is not the last gets max(0, first index of the next - its own)).
 *                                sqrt(noise_size) is rounded to float32 in both dtypes, as torch.sqrt of the reference's int64 tensor is.
 *                                Nothing between the rows and the response leaves LDS.
 *   dsa_world_synth_overlap_add  world_synth.py:302-315: y:(B,T), T <= N P the output length; y[b,j] = the responses of utterance b that
 *                                cover sample j + L / 2 of the padded waveform, added in ascending pulse order (a bisection over the
 *                                sorted indices, one thread per sample).
 *   dsa_world_synth_vjp_pulses   one workgroup per pulse: the forward again, the response's cotangent read from gy:(B,T) (zero outside it),
 *                                the adjoint down to grows:(pulses,2,D) = the cotangents of the interpolated sp row and of the
 *                                interpolated ap row (before squaring).
 *   dsa_world_synth_vjp_frames   one workgroup per frame: gsp, gap:(B,N,D), every element written: the pulses whose floor or ceil frame
 *                                it is (one run, by bisection) added in pulse order with the lower / upper weights; exactly zero where
 *                                sp < 1e-6 or ap outside [1e-6, 1 - 1e-6].  No gradient reaches f0 (the reference detaches it).
 * The host layer draws the noise with the device's generator (for one seed other numbers than the reference's CPU generator).  A call in
 * which no pulse falls anywhere returns zeros: pulses = 0 launches nothing per pulse and the overlap-add writes zeros (the reference
 * fails there inside its FFT).
 * dsa_last_kernel(): "world_synth_pulses_f32", "world_synth_responses_f32", "world_synth_overlap_add_f32", "world_synth_vjp_pulses_f32",
 * "world_synth_vjp_frames_f32" and the same with f64.
 * DSA_ERR_INVALID_ARGUMENT with a message that names "world_synth": a negative size, B beyond 65535, N P beyond 2^24 in float32 (the time axis
 * is exact up to there) or beyond int32, an unknown dtype, a missing pointer, an L that is no power of two (the reference takes any
 * L >= 1024; WORLD itself uses powers of two), and DSA_WORLD_LDS_BYTES(L, sizeof(dtype)) > DSA_WORLD_MAX_LDS_BYTES: the per-pulse
 * workgroup holds one complex transform of L points, the two half spectra it carries (4 (L / 2 + 1) values) and its reductions'
 * exchange in LDS (float32: L <= 8192, float64: L <= 4096). */
#define DSA_WORLD_MAX_LDS_BYTES 163840
#define DSA_WORLD_LDS_BYTES(L, size) ((4 * (L) + 4) * (size) + 256)
int dsa_world_synth_pulses(const void* f0, int64_t B, int64_t N, int32_t P, int32_t sample_rate, int32_t L, double default_f0, const void* offsets,
                           int32_t dtype, void* counts, void* irec, void* frec, void* stream);
int dsa_world_synth_responses(const void* ap, const void* sp, const void* noise, const void* irec, const void* frec, const void* offsets,
                              const void* dc_remover, const void* twiddle, int64_t B, int64_t N, int32_t sample_rate, int32_t L, int64_t pulses,
                              int32_t dtype, void* response, void* stream);
int dsa_world_synth_overlap_add(const void* response, const void* irec, const void* offsets, int64_t B, int64_t T, int32_t L, int64_t pulses,
                                int32_t dtype, void* y, void* stream);
int dsa_world_synth_vjp_pulses(const void* gy, const void* ap, const void* sp, const void* noise, const void* irec, const void* frec,
                               const void* offsets, const void* dc_remover, const void* twiddle, int64_t B, int64_t N, int64_t T,
                               int32_t sample_rate, int32_t L, int64_t pulses, int32_t dtype, void* grows, void* stream);
int dsa_world_synth_vjp_frames(const void* grows, const void* ap, const void* sp, const void* irec, const void* frec, const void* offsets, int64_t B,
                               int64_t N, int32_t L, int64_t pulses, int32_t dtype, void* gap, void* gsp, void* stream);

/* ------------------------------------------------------------------ a25  Band aperiodicity by TANDEM-STRAIGHT: ap (0.4.0)
 * AperiodicityExtractionByTANDEM.forward, ap.py:294-374, with the clip and the output format of Aperiodicity.forward, ap.py:166-167.
 * x:(B,T) and f0:(B,N) in Hz, of the dtype (float32 or float64); N is f0's own, not tied to T / P.  n_band = int(log2(sample_rate / 600))
 * <= DSA_AP_MAX_BANDS; band i has cutoff_i = sample_rate / 2^min(i + 2, n_band), tmp_fs_i = 2 cutoff_i, the segment
 * J_i = int(cutoff_i window_length_ms / 500 + 1.5) and T_i samples, T_0 = ceil(T / 2), T_(i+1) = ceil(T_i / 2), the last band as long as
 * the one before it.  `bands`:(B,ldb) holds them side by side in a row, band i from column sum_{k<i} T_k on, in FLOAT64 whatever the dtype,
 * as are their cotangents gbands: on a clean periodic signal the aperiodicity is the rounding noise of the band signals (float32 bands, or
 * the taps rounded to float32, each moved a float32 sinusoid's result by 1e-5; the float32 window: 3e-9).  int64 indexing, no
 * allocation, no host synchronisation, no atomics: every sum has one fixed order, two runs give the same bits, and an utterance's bits
 * are those of the utterance run alone.  B = 0 (and N = 0, T = 0 where nothing is to be written) is a no-op before any pointer is
 * looked at.
 *   dsa_ap_qmf         one level of the pyramid (ap.py:304-310): from x:(B,T) of the dtype with row stride ldx (the waveform; a deeper level
 *                      is float64: dtype = DSA_F64), hp, lp:(B, ceil(T / 2)) float64 with their row strides: the 41-tap high-pass and the
 *                      37-tap low-pass of ap.py:376-424 (float64 constants of the library; the module's hHP / hLP buffers hold the same
 *                      values in its dtype) at stride 2 over the input reflected by 20 / 18 samples; T >= 21.  The taps are added in
 *                      ascending order.
 *   dsa_ap_qmf_vjp     its transpose: gx:(B,T) of the dtype, every element written, = the taps of ghp and glp:(B, ceil(T / 2)), float64,
 *                      that read the sample, directly and through the two reflections, in that order.
 *   dsa_ap_tandem      y:(B,N,K).  One workgroup per (utterance, frame), one wave per band.  Per band the decisions
 *                      pitch = tmp_fs / f0 (f0 <= 32 reads as 150), t0 = int(pitch + 0.5), index_bias = int(pitch 0.5 + 0.5),
 *                      curr_pos = int(fl(fl(n fl(P / sr)) tmp_fs) + 1.5), every operation rounded on its own in the dtype; three runs of
 *                      J + 2 samples from curr_pos - index_bias - 1 -/+ t0 and from curr_pos - index_bias - 1, indices clamped to the band;
 *                      R = H' W H, b = H' W X with the window:(n_band,ldw) rows of the module; a = (R + eps m I)^-1 b by Cholesky with
 *                      m = 1, 10, ... 10^8, the first m at which every pivot is positive and finite -- PER FIT (the reference escalates
 *                      the whole batch together, so there a frame depends on its neighbours); A = std(sqrt(w) (X - H a)) /
 *                      (std(sqrt(w) X) + 1e-16), unbiased, sqrt(w) = window_sqrt; a fit that no m factors gives upper_bound (the reference
 *                      raises).  The sums, the factorisation and the stds run in float64 for both dtypes, so a float32 fit escalates only
 *                      where a float64 one does.  Then the lowest band doubled, the order reversed; with interp_indices:(K) int64 and
 *                      interp_weights:(K) of the dtype, K = L / 2 + 1, exp(log A[i] + w (log A[i + 1] - log A[i])) -- 0 where one of the
 *                      two is exactly 0 (the reference: NaN from log 0) --, with both NULL the K = n_band + 1 band values; clipped to
 *                      [lower_bound, upper_bound]; out_format 0 a, 1 1 - a, 2 a / (1 - a), 3 (1 - a) / a.
 *   dsa_ap_tandem_vjp  gbands:(B,ldg) float64, every band sample written, for the cotangent gy:(B,N,K): the fits again, the adjoint of the
 *                      epilogue (nothing passes a clipped or silent bin), the stds (a zero-variance denominator: no gradient), the
 *                      residual and the regularised solve (eps m I a constant) into gruns:(B,N,3 sum(J + 2)) of the dtype, the run starts
 *                      curr_pos and the number of failed trials (m = 10^that; 9 = none factored) into
 *                      starts:(B,N,n_band,DSA_AP_START_WORDS) int64 -- both scratch of the caller --, then a second launch: one thread per
 *                      band sample adds the run elements that read it in ascending (frame, run) order -- curr_pos does not decrease with
 *                      n, so the frames are one range, found by bisection --, and a workgroup each adds what the clamp piled onto samples
 *                      0 and T_i - 1.  No gradient reaches f0 (the reference detaches it).
 * dsa_last_kernel(): "ap_qmf_f32", "ap_qmf_vjp_f32", "ap_tandem_f32", "ap_tandem_vjp_f32" and the same with f64.
 * DSA_ERR_INVALID_ARGUMENT with a message that names "ap": a negative size, B beyond 65535, N beyond 2^24 in float32 (the frame index is
 * exact up to there) or beyond int32, a level shorter than 21 samples, rows too short for their bands, options outside their ranges, an
 * unknown dtype, a missing pointer, n_band > DSA_AP_MAX_BANDS and DSA_AP_LDS_BYTES(sum(J), n_band) > DSA_AP_MAX_LDS_BYTES: the workgroup
 * holds, in float64, the three runs of every band and two more arrays of J + 2 for the adjoint (the same ceiling forward and backward;
 * with window_length_ms = 30 up to sample_rate = 135699; 96 kHz takes 116168 bytes). */
#define DSA_AP_MAX_BANDS 8
#define DSA_AP_START_WORDS 5
#define DSA_AP_MAX_LDS_BYTES 163840
#define DSA_AP_LDS_BYTES(S, n_band) (40 * ((S) + 2 * (n_band)) + 128)
int dsa_ap_qmf(const void* x, int64_t B, int64_t T, int64_t ldx, int32_t dtype, void* hp, int64_t ldhp, void* lp, int64_t ldlp, void* stream);
int dsa_ap_qmf_vjp(const void* ghp, int64_t ldghp, const void* glp, int64_t ldglp, int64_t B, int64_t T, int32_t dtype, void* gx, int64_t ldgx,
                   void* stream);
int dsa_ap_tandem(const void* bands, int64_t ldb, const void* f0, const void* window, const void* window_sqrt, int64_t ldw,
                  const void* interp_indices, const void* interp_weights, int64_t B, int64_t N, int64_t T, int32_t P, int32_t sample_rate,
                  double window_length_ms, int32_t K, double eps, double lower_bound, double upper_bound, int32_t out_format, int32_t dtype,
                  void* y, void* stream);
int dsa_ap_tandem_vjp(const void* gy, const void* bands, int64_t ldb, const void* f0, const void* window, const void* window_sqrt, int64_t ldw,
                      const void* interp_indices, const void* interp_weights, int64_t B, int64_t N, int64_t T, int32_t P, int32_t sample_rate,
                      double window_length_ms, int32_t K, double eps, double lower_bound, double upper_bound, int32_t out_format, int32_t dtype,
                      void* gruns, void* starts, void* gbands, int64_t ldg, void* stream);

/* ------------------------------------------------------------------ a26  Pitch-adaptive spectral envelope (CheapTrick): pitch_spec (0.4.1)
 * SpectrumExtractionByCheapTrick.forward, pitch_spec.py:257-304, with the formatter of pitch_spec.py:158-168.  x:(B,T) and f0:(B,N) in Hz, of
 * the dtype (float32 or float64), N = (T - 1) / P + 1; noise1:(B,N,L) and noise2:(B,N,K), K = L / 2 + 1, of the dtype: the standard normal
 * numbers of the reference's two randn_like calls (either may be NULL: no noise); twiddle:(L,2) FLOAT64 = (cos, -sin)(2 pi m / L) whatever
 * the dtype.  Per frame, with f = default_f0 where f0 <= f_min = 3 sample_rate / (L - 3), rate = sample_rate / L:
 *   1 window     h = round(1.5 sample_rate / f), ties to even; w[i] = 0.5 + 0.5 cos(pi j f / (1.5 sample_rate)) on |j| <= h, j = i - L / 2,
 *                over its L2 norm
 *   2 frame      u = x[clamp(n P + j, 0, T - 1)] w + 1e-12 noise1 [|j| <= h];  s = u - w sum(u) / sum(w)
 *   3 power      A = |FFT(s)|^2 + eps;  max(A, max(A) floor_ratio) when floor_ratio > 0 (= 10^(relative_floor / 10))
 *   4 DC         bins with k rate < f add the spectrum read linearly at (f - k rate) / rate
 *   5 smoothing  the spectrum mirrored by b = trunc(2 f / (3 rate)) + 1 bins on both sides, times rate, summed from the frame's own first
 *                element (the reference starts at the widest boundary of the BATCH, after a host read), read linearly at
 *                k + b - 1/2 -/+ f / (3 rate); the difference over 2 f / 3
 *   6 noise      + |noise2| 2^-52: finfo(float64).eps for BOTH dtypes, the arithmetic being float64 (the reference's float32 run adds
 *                |noise2| 2^-23, which alone moves its result by 1e-5 .. 3e-4 of the largest value)
 *   7 liftering  irfft(log .)[:K] times sinc(f q) ((1 - 2 q1) + 2 q1 cos(2 pi f q)), q = k / sample_rate, then hfft(.)[:K]
 *   8 format     out_format 0 db: 10 / ln 10 times it, 1 log-magnitude: half of it, 2 magnitude: exp of half, 3 power: exp
 * Everything from the loaded sample to the formatted value runs in float64 for both dtypes: a float32 call returns the float64 result
 * rounded once.  The integers (h, the DC mask, the truncations of the reads, f0 <= f_min) are evaluated in float64 from the stored values; a
 * read's position is truncated once per frame (bin k reads k bins further), which is continuous across the reference's truncations.
 * F0 must stay below sample_rate / 2 (the reference fails in a gather there; here the reads are clamped and the values are unspecified).
 * int64 indexing, no allocation, no host synchronisation, no atomics: two runs give the same bits, and a frame's bits are those of the
 * frame run alone.  B, N or T of 0 is a no-op before any pointer is looked at.
 *   dsa_pitch_spec             y:(B,N,K) of the dtype.  One workgroup per frame, one launch.
 *   dsa_pitch_spec_vjp_frames  gframes:(B,N,L) FLOAT64, scratch of the caller, every element written: the forward again, then the adjoint of
 *                              the eight steps for the cotangent gy:(B,N,K); a frame's row is zero outside |j| <= h.  No gradient reaches f0.
 *   dsa_pitch_spec_vjp_gather  gx:(B,T) of the dtype, every element written: one thread per sample adds, in ascending frame order, the frames
 *                              that cover it; samples 0 and T - 1 also collect what the replicate padding sent to them, a workgroup each.
 *                              T = 1 (one frame): the padding clamps all L columns to the one sample, and gx is their sum (since 0.4.2).
 * dsa_last_kernel(): "pitch_spec_f32", "pitch_spec_vjp_frames_f32", "pitch_spec_vjp_gather_f32" and the same with f64.
 * DSA_ERR_INVALID_ARGUMENT with a message that names "pitch_spec": a negative size, an unknown dtype, an L that is no power of two (the
 * reference takes any length >= 1024; WORLD itself uses powers of two) or below 16, DSA_PITCH_SPEC_LDS_BYTES(L) >
 * DSA_PITCH_SPEC_MAX_LDS_BYTES (the workgroup holds, in float64, a complex transform of L points, the kept spectrum and the smoothed
 * spectrum: L <= 4096, which serves 96 kHz; 8192 is refused), N other than (T - 1) / P + 1, B beyond 65535 or B N beyond int32, options
 * outside their ranges, a missing pointer. */
#define DSA_PITCH_SPEC_MAX_LDS_BYTES 163840
#define DSA_PITCH_SPEC_LDS_BYTES(L) (28 * (L) + 280)
int dsa_pitch_spec(const void* x, const void* f0, const void* noise1, const void* noise2, const void* twiddle, int64_t B, int64_t N, int64_t T,
                   int32_t P, int32_t sample_rate, int32_t L, double default_f0, double q1, double eps, double floor_ratio, int32_t out_format,
                   int32_t dtype, void* y, void* stream);
int dsa_pitch_spec_vjp_frames(const void* gy, const void* x, const void* f0, const void* noise1, const void* noise2, const void* twiddle, int64_t B,
                              int64_t N, int64_t T, int32_t P, int32_t sample_rate, int32_t L, double default_f0, double q1, double eps,
                              double floor_ratio, int32_t out_format, int32_t dtype, void* gframes, void* stream);
int dsa_pitch_spec_vjp_gather(const void* gframes, int64_t B, int64_t N, int64_t T, int32_t P, int32_t L, int32_t dtype, void* gx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSPTK_AMD_H */
