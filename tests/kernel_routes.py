"""The kernel routes' table, names and cases only.  A route is a name a host launcher hands to check_launch() after it picked one of
its kernels from the geometry and the dtype (diffsptk_amd/csrc/*.hip, *.h); `_lib.last_kernel()` reads it back.  Every route is in
exactly one of

  ROUTES            route -> cases that reach it through a public call and compare it with a float64 restatement
                    (tests/test_gpu_routes.py runs them; the restatements and the inputs are tests/routes_ref.py)
  PINNED_ELSEWHERE  route -> "tests/<file>.py::<test function>" that already asserts the name through last_kernel()
  EXEMPT            route -> why no case can name it (at most 5)

The names are the string literals inside the parentheses of a check_launch(...) call and the literals of every name table of the
sources (`const char* const k<Name>Routes[...]` / `k<Name>Names[...]`, which a launcher indexes on its way to check_launch());
FORWARDED lists the few that reach check_launch() as a function argument or through a local, with the function that spells them.
Every pointer into the sources is "csrc/<file>::<function>", the host function that encloses the site, never a line number: an
edit elsewhere in the file leaves it valid, and a renamed or removed function fails by the row's name.
tests/test_routes_cpu.py checks, without a GPU, that nothing is missing, stale or in two places.  The same discipline holds the other
end of every launcher: each DSA_ERR_UNSUPPORTED of the sources is claimed by exactly one of REFUSALS (the first refused shapes of
csrc/lpc.hip), CEILINGS (every size condition that refuses or silently reshapes a launch: the last shape in by float64, the first
shape out by message or by route) and NOT_A_CEILING (message -> why no size a caller can reach meets it).

A case: the call (a key of CALLS in tests/test_gpu_routes.py and of INPUTS / REFS in tests/routes_ref.py), whether the name is read
after the forward ("fwd") or on autograd's thread after the backward ("bwd", with the inputs `wrt` whose gradients are compared),
the dtypes the route is instantiated for, the arguments (shapes and options: the smallest that satisfy the launcher's condition,
and the nearest shape on the other side of it under the neighbouring route), and the tolerance with where it comes from:

  tol_from = "measured"     (base64, base32) of MEASURED[case id], measured on the CPU from the restatement alone
                            (tests/routes_ref.py: `python tests/routes_ref.py` prints them):
                                float64  64 x max(base64, 2^-53)    base64 = two float64 evaluations, opposite summation order
                                float32   8 x max(base32, 2^-24)    base32 = the restatement in float32 against float64
  tol_from = "tests/..."    the bound of an existing test that compares the same entry with a reference, as (float64, float32)

Errors are relative to the largest |reference| entry of the compared tensor ("max"), or of each row ("rows") where the cited test
judges rows."""

U64, U32 = 2.0 ** -53, 2.0 ** -24
BOTH, F64, F32 = ("f64", "f32"), ("f64",), ("f32",)
MEAS = "measured"


def case(call, when, dtypes=BOTH, wrt=(), tol=None, tol_from=MEAS, metric="max", **args):
    assert (tol is None) == (tol_from == MEAS)
    return {"call": call, "when": when, "dtypes": dtypes, "wrt": tuple(wrt), "tol": tol, "tol_from": tol_from, "metric": metric, "args": args}


def case_id(route, c):
    return "-".join([route, c["call"], c["when"]] + [f"{k}{v}" for k, v in c["args"].items()] + (["only" + c["dtypes"][0]] if len(c["dtypes"]) == 1 else []))


def tolerance(route, c, dt):
    """the bound of case c in dtype dt ("f64" / "f32")"""
    if c["tol_from"] != MEAS:
        return c["tol"][dt == "f32"]
    b64, b32 = MEASURED[case_id(route, c)]
    return 8 * max(b32, U32) if dt == "f32" else 64 * max(b64, U64)


def both(call, wrt, **kw):
    """the forward case and the backward case of one set of arguments"""
    return [case(call, "fwd", **kw), case(call, "bwd", wrt=wrt, **kw)]


ZDF_FWD = dict(tol=(1e-11, 3e-5), tol_from="tests/test_gpu_synth.py::test_zerodf_and_linear_intpl")
ZDF_BWD = dict(tol=(1e-11, 2e-5), tol_from="tests/test_gpu_synth.py::test_zerodf_backward_kernels_against_autograd_of_the_definition")
PQ = dict(tol=(1e-12, 1e-5), tol_from="tests/test_gpu_pqmf.py::test_reference_goldens")
FFTCEP = dict(tol=(1e-9, 5e-4), metric="rows", tol_from="tests/test_gpu_parity.py::test_fftcep_golden_forward_backward")
MCEP_X = dict(tol=(1e-6, 2e-3), metric="rows", tol_from="tests/test_gpu_parity.py::test_mcep_backward_wrt_spectrum_golden")
MCEP_T = dict(tol=(None, 3.5e-6), tol_from="tests/test_gpu_configs.py::test_mcep_backward_two_waves_per_simd_against_the_one_wave_kernel_and_float64")
GC = dict(tol=(1e-10, 2e-4), tol_from="tests/test_gpu_synth.py::test_gc2gc_backward_kernel_against_autograd_of_the_definition")
PLP_OUT = dict(tol=(1e-10, 2e-5), tol_from="tests/test_gpu_plp.py::test_reference_goldens")
PLP_GRAD = dict(tol=(1e-8, 2e-3), tol_from="tests/test_gpu_plp.py::test_reference_goldens")

ACORR = [(L, M, fmt) for L in (1, 63, 64, 65, 257) for M in sorted({0, min(7, L - 1), L - 1}) for fmt in range(4)]   # 7 lags: more than the block's 4 waves
FFTR = [(ln, n, 0) for n in (12, 16, 30, 32, 64) for ln in (n // 2, n, n + 5)] + [(n + 5, n, fmt) for n in (30, 32) for fmt in (1, 2, 3, 4)]


def direct(n):   # launch_row_dft (csrc/spec.hip): the radix-2 FFT in LDS takes the powers of two from 32 on, the direct sum the rest
    return n < 32 or n & (n - 1) != 0


ROUTES = {
    # ---- csrc/lpc.hip.  levdur_fwd_impl: M <= 63 in registers (lane 63 owns a_63 at the edge), above with a[] in LDS
    "levdur_fwd": [case("levdur", "fwd", M=M, eps=eps) for M in (0, 1, 62, 63) for eps in (0.0, 1e-5)],
    "levdur_fwd_lds": [case("levdur", "fwd", M=M, eps=eps) for M in (64, 65, 100) for eps in (0.0, 1e-5)]
                      + [case("lpc", "fwd", L=404, M=100, eps=1e-5)],   # LPC(frame_length, lpc_order = 100): acorr_fwd, then this
    # levdur_bwd_impl: the dense solve while M (M + 1) doubles fit 60 KB of LDS (M <= 85), the Toeplitz solve above (to M = 1097)
    "levdur_bwd": [case("levdur", "bwd", wrt=("r",), M=M, eps=1e-5) for M in (1, 24, 63, 64, 85)],
    "levdur_bwd_toeplitz": [case("levdur", "bwd", wrt=("r",), M=M, eps=1e-5) for M in (86, 100)],
    "acorr_fwd": [case("acorr", "fwd", L=L, M=M, fmt=fmt) for L, M, fmt in ACORR],
    # (normalized with M = 0 is the constant 1: its gradient is zero and has no scale to be relative to)
    "acorr_bwd": [case("acorr", "bwd", wrt=("x",), L=L, M=M, fmt=fmt) for L, M, fmt in ACORR if not (fmt == 1 and M == 0)]
                 # the backward of LPC at orders past the dense solve: acorr_fwd, levdur_bwd_toeplitz, and this as its last launch
                 + [case("lpc", "bwd", wrt=("x",), L=4 * (M + 1), M=M, eps=1e-5) for M in (86, 100)],
    # dsa_frame_window_lpc_fwd: float32 at order 24 with 25 <= L <= 512 goes to the tuned kernels, everything else to the generic
    # fused kernel (4 frames per block: 26 frames leave a partial block); exact_lag_sums picks the tuned kernel with float64 lag sums
    "frame_window_lpc_fwd": [case("fwlpc", "fwd", F64, T=250, L=50, P=20, M=24, eps=1e-5),
                             case("fwlpc", "fwd", F32, T=250, L=50, P=20, M=23, eps=1e-5),
                             case("fwlpc", "fwd", BOTH, T=250, L=64, P=20, M=63, eps=1e-5, center=False)],
    "frame_window_lpc24_fwd": [case("fwlpc", "fwd", F32, T=250, L=50, P=20, M=24, eps=1e-5, exact=True)],
    # ---- csrc/zerodf.hip.  zerodf_launch_fwd: rows (P % 4 == 0, M >= 16), blocked (M >= 64, 4 <= P <= 128), sliced (M >= 64, P <= 3)
    "zerodf_sliced_fwd": [case("zerodf", "fwd", M=M, P=P, z0=z0, ig=ig, N=N, **ZDF_FWD)
                          for M, P, z0, ig, N in ((64, 1, 0, False, 7), (70, 3, 5, True, 5), (129, 2, 129, False, 4))],
    "zerodf_blocked_fwd": [case("zerodf", "fwd", M=70, P=5, z0=5, ig=True, N=5, **ZDF_FWD)],
    "zerodf_rows_fwd": [case("zerodf", "fwd", M=64, P=4, z0=0, ig=False, N=7, **ZDF_FWD)],
    "zerodf_fwd": [case("zerodf", "fwd", M=63, P=3, z0=5, ig=True, N=5, **ZDF_FWD)],
    # zerodf_launch_bwd: the rows kernels without ignore_gain at P % 4 == 0 and M >= 16, the first kernels otherwise
    "zerodf_bwd": [case("zerodf", "bwd", wrt=("x", "b"), M=M, P=P, z0=z0, ig=ig, N=5, **ZDF_BWD)
                   for M, P, z0, ig in ((20, 8, 0, True), (20, 6, 3, False), (15, 8, 15, False))],
    "zerodf_rows_bwd": [case("zerodf", "bwd", wrt=("x", "b"), M=M, P=8, z0=z0, ig=False, N=5, **ZDF_BWD) for M, z0 in ((20, 0), (16, 16))],
    # ---- csrc/spec.hip.  launch_row_dft / launch_row_dft_bwd: zero-padded, exact and cropped rows either side of nfft = 32
    "row_dft_generic": [case("fftr", "fwd", len_in=ln, nfft=n, fmt=fmt) for ln, n, fmt in FFTR if direct(n)]
                       + [case("spec", "fwd", lb=35, la=0, nfft=30, eps=1e-6, floor=-20.0, fmt=0),
                          case("stft", "fwd", T=100, L=20, P=7, nfft=30)],
    "row_fft_generic": [case("fftr", "fwd", len_in=ln, nfft=n, fmt=fmt) for ln, n, fmt in FFTR if not direct(n)]
                       + [case("spec", "fwd", lb=37, la=0, nfft=32, eps=1e-6, floor=-20.0, fmt=0),
                          case("stft", "fwd", T=100, L=20, P=7, nfft=32)],
    "row_dft_bwd_generic": [case("fftr", "bwd", wrt=("x",), len_in=ln, nfft=n, fmt=fmt) for ln, n, fmt in FFTR if direct(n)]
                           + [case("spec", "bwd", wrt=("b",), lb=35, la=0, nfft=30, eps=1e-6, floor=-20.0, fmt=0)],
    "row_fft_bwd_generic": [case("fftr", "bwd", wrt=("x",), len_in=ln, nfft=n, fmt=fmt) for ln, n, fmt in FFTR if not direct(n)]
                           + [case("spec", "bwd", wrt=("b",), lb=37, la=0, nfft=32, eps=1e-6, floor=-20.0, fmt=0)],
    "spec_ratio": [case("spec", "fwd", lb=5, la=3, nfft=16, eps=1e-3, floor=None, fmt=3),
                   case("spec", "fwd", lb=3, la=6, nfft=30, eps=0.0, floor=None, fmt=0),
                   case("spec", "fwd", lb=0, la=4, nfft=16, eps=0.0, floor=-30.0, fmt=1)],
    "spec_ratio_bwd": [case("spec", "bwd", wrt=("b", "a"), lb=5, la=3, nfft=16, eps=1e-3, floor=None, fmt=3),
                       case("spec", "bwd", wrt=("b", "a"), lb=3, la=6, nfft=30, eps=0.0, floor=None, fmt=0),
                       case("spec", "bwd", wrt=("a",), lb=0, la=4, nfft=16, eps=0.0, floor=-30.0, fmt=1)],
    # a learnable window: its gradient is the column sum over the 2 x 15 frames (not a multiple of the 256-thread block)
    "window_grad_colsum": [case("stft", "bwd", wrt=("x", "w"), T=100, L=20, P=7, nfft=n) for n in (30, 32)],
    "irfft_scale": [case("irfft_scale", "fwd", nfft=n) for n in (2, 30)],
    # ---- csrc/thsolve.hip.  dsa_thsolve_bwd: float32 order 24, float32 orders 2 .. 55, and the one-wave kernel for the rest
    "th_solve_bwd": [case("thsolve", "bwd", F64, wrt=("p", "q", "r"), n=n) for n in (1, 24, 25, 64)]
                    + [case("thsolve", "bwd", F32, wrt=("p", "q", "r"), n=n) for n in (1, 56, 64)],
    "th_solve_quad_bwd": [case("thsolve", "bwd", F32, wrt=("p", "q", "r"), n=24)],
    "th_solve_quadn_bwd": [case("thsolve", "bwd", F32, wrt=("p", "q", "r"), n=n) for n in (2, 23, 25, 55)],
    # ---- csrc/mcep.hip, row products.  dsa_freqt_fwd: float32 rows of 49 .. 320 on the matrix cores, else the LDS-resident kernel
    # while the matrix and 64 rows fit 48 KB, else one workgroup per row; dsa_freqt_bwd: the last two
    "freqt_lds_fwd": [case("freqt", "fwd", BOTH, L1=48, L2=25), case("freqt", "fwd", F64, L1=49, L2=25)],
    "freqt_mfma_fwd": [case("freqt", "fwd", F32, L1=49, L2=25, tol=(None, 2e-5),
                            tol_from="tests/test_gpu_configs.py::test_long_row_products_on_matrix_cores")],
    "freqt_fwd": [case("freqt", "fwd", F32, L1=400, L2=40), case("freqt", "fwd", F64, L1=100, L2=70)],
    "freqt_lds_bwd": [case("freqt", "bwd", BOTH, wrt=("c",), L1=48, L2=25), case("freqt", "bwd", BOTH, wrt=("c",), L1=49, L2=25)],
    "freqt_bwd": [case("freqt", "bwd", F32, wrt=("c",), L1=400, L2=40), case("freqt", "bwd", F64, wrt=("c",), L1=100, L2=70)],
    "rows_log": both("rows_log", ("x",), dtypes=F32, n=300),
    "rows_expsub": both("rows_expsub", ("a", "b"), dtypes=F32, n=300),
    # ---- csrc/fftcep.hip.  fftcep_launch: the FFT in LDS with iterations at a power-of-two length from 32 on, else the cosine matrix
    "fftcep_fft_bwd": [case("fftcep", "bwd", wrt=("x",), nfft=32, M=5, accel=0.5, n_iter=2, **FFTCEP)],
    "fftcep_bwd": [case("fftcep", "bwd", wrt=("x",), nfft=n, M=5, accel=a, n_iter=i, **FFTCEP) for n, a, i in ((32, 0.0, 0), (30, 0.5, 2), (30, 0.0, 0))],
    # ---- csrc/fbank.hip
    "fbank_bwd": [case("fbank", "bwd", wrt=("x",), nfft=64, C=12, use_power=p, gamma=g) for p, g in ((False, 0.0), (True, -0.5))],
    # (float32 only: the fused STFT -> filter bank it differentiates is)
    "fbank_bins_bwd": [case("fbank_bins", "bwd", F32, wrt=("s",), nfft=64, C=12, gamma=g) for g in (0.0, -0.5)],
    # ---- csrc/mgc.hip
    "gc2gc_fused_bwd": [case("gc2gc", "bwd", wrt=("c",), g1=g1, g2=g2, n_fft=64, m1=8, m2=12, **GC) for g1, g2 in ((-0.5, 0.0), (0.0, -0.5))],
    "mgcep_step": [case("mgcep_step", "fwd", F32, nfft=512, M=M, gamma=-0.5) for M in (24, 17)],
    "mgcep_step_bwd": [case("mgcep_step", "bwd", F32, wrt=("x", "b1"), nfft=512, M=17, gamma=-0.5)],
    "mgcep_spectra": [case("mgcep_spectra", "fwd", nfft=64, M=M, gamma=-0.5) for M in (8, 32)],
    "mgcep_gain": [case("mgcep_gain", "fwd", M=M, gamma=-0.5) for M in (1, 24)],
    # ---- the mel-cepstral kernels: their existing tests' tolerances, nothing more
    "mcep_generic_bwd": [case("mcep", "bwd", wrt=("X",), nfft=64, M=8, alpha=0.42, n_iter=2, **MCEP_X)],
    "mcep_mfma_bwd2": [case("mcep_tuned", "bwd", F32, wrt=("X",), n_iter=10, keep_rt=True, **MCEP_T)],
    "mcep_mfma_bwd": [case("mcep_tuned", "bwd", F32, wrt=("X",), n_iter=10, keep_rt=False, **MCEP_T)],
    "mcep_newton_update_bwd": [case("newton_update", "bwd", F32, wrt=("rt",), n=n) for n in (7, 35)],
    "mcep_glogx_h": [case("glogx", "fwd", F32, K=37, n=33, n_iter=3, F=5, tol=(None, 2e-6), metric="rows",
                          tol_from="tests/test_gpu_48k_grad.py::test_glogx_entry_against_float64_of_its_formula_and_null_glogx_in_the_sweep")],
    # ---- csrc/poledf.hip, pqmf.hip, plp.hip, paramgen.hip, mdct.hip
    "poledf_generic_bwd": [case("poledf", "bwd", wrt=("x",), M=M, P=16, N=3, ig=ig) for M, ig in ((0, False), (64, True))],
    # pqmf_launch_bwd / ipqmf_launch_bwd: the tuned kernels at K <= 8, M <= 127, period 1, start 0
    "pqmf_bwd_x_tuned": [case("pqmf", "bwd", wrt=("x",), K=4, M=40, T=300, **PQ)],
    "pqmf_bwd_x": [case("pqmf", "bwd", wrt=("x",), K=9, M=40, T=300, **PQ), case("pqmf", "bwd", wrt=("x",), K=4, M=41, T=300, P=3, s=1, **PQ)],
    "pqmf_f_sum": [case("pqmf", "bwd", wrt=("x", "f"), K=3, M=7, T=300, P=2, s=1, **PQ), case("ipqmf", "bwd", wrt=("y", "f"), K=3, M=7, T=70, U=2, s=1, **PQ)],
    "ipqmf_bwd_y_tuned": [case("ipqmf", "bwd", wrt=("y",), K=4, M=40, T=70, **PQ)],
    "ipqmf_bwd_y": [case("ipqmf", "bwd", wrt=("y",), K=9, M=40, T=70, **PQ), case("ipqmf", "bwd", wrt=("y",), K=4, M=41, T=70, U=3, s=1, **PQ)],
    "interpolate_fwd": [case("interpolate", "fwd", T=7, P=3, s=2)],
    "interpolate_bwd": [case("interpolate", "bwd", wrt=("x",), T=7, P=3, s=2)],
    "plp_fwd": [case("plp_tail", "fwd", C=20, M=12, n_fft=64, **PLP_OUT)],
    "plp_bwd": [case("plp_tail", "bwd", wrt=("y", "E"), C=20, M=12, n_fft=64, **PLP_GRAD)],
    "delta_bwd": [case("delta", "bwd", wrt=("x",), T=9, D=3, seed="w23")],
    # dsa_mlpg: bands of more than DSA_MLPG_MAX_REGISTER_BAND = 8 off-diagonals (window half-width 5) leave the register kernels
    "mlpg_adjoint_any": [case("mlpg", "bwd", wrt=("u",), T=30, D=3, seed="w5")],
    # dsa_mdct_*: the fast kernels for float32 at a power-of-two length from 16 to 4096
    "mdct_analysis_fast": [case("mdct", "fwd", F32, L=16, T=50)],
    "mdct_analysis_generic": [case("mdct", "fwd", F64, L=16, T=50), case("mdct", "fwd", BOTH, L=12, T=50)],
    "mdct_synthesis_fast": [case("imdct", "fwd", F32, L=16, N=7)],
    "mdct_synthesis_generic": [case("imdct", "fwd", F64, L=16, N=7), case("imdct", "fwd", BOTH, L=12, N=7)],
}

# the four refusals of csrc/lpc.hip (DSA_ERR_UNSUPPORTED): call, arguments, dtype, forward or backward, and the launcher's message
REFUSALS = [
    ("levdur", dict(M=2560, eps=1e-5, F=1), "f64", "fwd", "levdur: order too large for LDS"),
    ("acorr", dict(L=7681, M=2, fmt=0, F=1), "f64", "fwd", "acorr: frame too long for LDS"),
    ("acorr", dict(L=15361, M=2, fmt=0, F=1), "f32", "fwd", "acorr: frame too long for LDS"),
    ("fwlpc", dict(T=300, L=100, P=40, M=64, eps=1e-5, B=1), "f32", "fwd", "frame_window_lpc: fused kernel supports lpc_order <= 63"),
    ("levdur", dict(M=1098, eps=1e-5, F=1), "f64", "bwd", "levdur_bwd: order too large for LDS"),
]

# ---- the size ceilings.  One row per size condition of csrc/*.hip / *.h that refuses a launch (DSA_ERR_UNSUPPORTED) or silently
# reshapes it (fewer waves per block, a table left in global memory, the direct sum instead of the FFT: the route name stays):
#   where     "csrc/<file>::<function>": the host function(s) that hold the condition
#   says      the launcher's message, or "reshapes: ..." and what changes
#   inside    (route, case) at the last accepted shape: every dtype, the forward, and the backward where there is one
#   outside   the nearest shape past the condition: raises(message, shape) -- BackendError from the forward, RuntimeError from autograd
#             for a backward whose forward ran -- or runs(route, case): that route runs instead and meets the same float64 comparison;
#             IN_REFUSALS: the first refused shape is a row of REFUSALS
#   shadowed  messages of the same condition in a backward launcher that the forward's refusal pre-empts (no call can show them)
# The GPU run of both sides (tests/test_gpu_routes.py) proves that they are adjacent; no LDS formula is restated in Python -- the
# arithmetic behind each shape is in the row's comment.  Batches are the smallest that use the launch's geometry.
IN_REFUSALS = "REFUSALS"


def shape(call, when, dtypes, wrt=(), **args):
    """a call that is only expected to raise: nothing is compared"""
    return case(call, when, dtypes, wrt=wrt, tol=(0.0, 0.0), tol_from="-", **args)


def raises(message, c, text=None):
    return {"expect": "raises", "message": message, "text": text or message, "case": c}


def runs(route, c):
    return {"expect": "route", "route": route, "case": c}


def ceiling(where, says, inside, outside, shadowed=(), cited=None):
    return {"where": (where,) if isinstance(where, str) else tuple(where), "says": says, "inside": inside, "outside": outside,
            "shadowed": tuple(shadowed), "cited": cited}


def per(pairs, make):
    """[make(dtypes, size) ...] for ((F32, size32), (F64, size64)): the shapes of a ceiling counted in bytes differ by dtype"""
    return [make(dt, n) for dt, n in pairs]


GCF = dict(tol=(1e-9, 5e-5), tol_from="tests/test_gpu_synth.py::test_gc2gc_fused_kernel_equals_the_operator_chain")
FBM = dict(tol=(None, 2e-5), tol_from="tests/test_gpu_parity.py::test_fbank_matrix_core_forward_matches_float64")
MFCC = dict(tol=(1e-8, 2e-4), tol_from="tests/test_gpu_parity.py::test_fbank_mfcc_golden_forward_backward")   # (its relative part)
ZDF_PIECES = "tests/test_gpu_mlsa_grad.py::test_a_filter_too_long_for_lds_is_the_sum_of_its_pieces"
AC, LD = dict(M=2, fmt=0, F=1), dict(eps=1e-5, F=1)
FW = dict(T=4000, P=2000, M=8, eps=1e-5, B=1)                    # 3 frames: one partial block of the fused kernel's 4
FB = dict(C=80, use_power=False, gamma=0.0, F=13)                # 4 groups of 4 frames, the last partial: 4 waves
FC0, FC2 = dict(M=5, accel=0.0, n_iter=0, F=2), dict(M=5, accel=0.5, n_iter=2, F=2)
PL = dict(C=20, M=12, F=5)                                       # 5 frames: more than the 4 waves of a block
SR = dict(lb=5, la=3, eps=1e-3, floor=None, fmt=3, F=2)
GE = dict(g1=-0.5, g2=0.0, m1=8, m2=12, F=2)
MG = dict(M=8, alpha=0.42, n_iter=2, F=2)
ZF, ZB = dict(P=3, z0=0, ig=True, N=2, B=1), dict(z0=0, ig=False, N=1, B=1)
E_ROW, E_ROWB = "row_dft: frame too long for LDS", "row_dft_bwd: frame too long for LDS"
E_FB, E_MC = "fbank: spectrum too long for LDS", "%s: the row and the bins do not fit the LDS"
E_PLP, E_PLPB = "plp: n_channel / n_fft too large for one wave's LDS", "plp_bwd: n_channel / n_fft too large for one wave's LDS"
E_GC, E_GCB = "gc2gc: unsupported dtype or n_fft too long for LDS", "gc2gc_bwd: unsupported dtype or n_fft too long for LDS"


def B32_64(n32, n64):
    return ((F32, n32), (F64, n64))


def mlsa_rows(mode, last_fwd, last_bwd, step, moves):
    """dsa_mlsacheck / _vjp at 2 (forward) and 3 (backward) rows of M + 1 doubles plus 2 K doubles against 144 KB: one row of the table
    per mode; `moves`: the argument that carries the size, its last forward and backward values, and its step.  Between the two
    values there is a forward and no gradient."""
    def a(v):
        return dict(dict(M=24, mode=mode, n_fft=256, F=3), **{moves: v})

    return ceiling("csrc/mlsacheck.hip::mlsacheck_generic_launch", E_MC,
                   inside=[("mlsacheck_generic_fwd", case("mlsacheck", "fwd", **a(last_fwd))),
                           ("mlsacheck_generic_bwd", case("mlsacheck", "bwd", wrt=("mc",), **a(last_bwd)))],
                   outside=[raises(E_MC, shape("mlsacheck", "fwd", BOTH, **a(last_fwd + step)), "mlsacheck_generic_fwd: the row and the bins"),
                            raises(E_MC, shape("mlsacheck", "bwd", BOTH, wrt=("mc",), **a(last_bwd + step)), "mlsacheck_generic_bwd: the row and the bins")])


def plp_waves(what, n32, n64):
    """a block of plp_fwd / plp_bwd goes from 4 waves to 2 to 1 as a wave's slice (8 (C + 194) + sizeof(T) (128 + 2 J), J = n_fft / 2 + 1)
    passes 16 KB and 32 KB: the last n_fft on one side, n_fft + 2 on the other, both under the same route name"""
    return ceiling("csrc/plp.hip::plp_geometry", "reshapes: " + what,
                   inside=per(B32_64(n32, n64), lambda dt, n: ("plp_fwd", case("plp_tail", "fwd", dt, n_fft=n, **PL, **PLP_OUT)))
                   + per(B32_64(n32, n64), lambda dt, n: ("plp_bwd", case("plp_tail", "bwd", dt, wrt=("y", "E"), n_fft=n, **PL))),
                   outside=per(B32_64(n32 + 2, n64 + 2), lambda dt, n: runs("plp_fwd", case("plp_tail", "fwd", dt, n_fft=n, **PL, **PLP_OUT)))
                   + per(B32_64(n32 + 2, n64 + 2), lambda dt, n: runs("plp_bwd", case("plp_tail", "bwd", dt, wrt=("y", "E"), n_fft=n, **PL))))


CEILINGS = [
    # ---- csrc/lpc.hip (60 KB of LDS each).  acorr_fwd keeps the frame: sizeof(T) L
    ceiling("csrc/lpc.hip::acorr_fwd_impl", "acorr: frame too long for LDS",
            inside=per(B32_64(15360, 7680), lambda dt, L: ("acorr_fwd", case("acorr", "fwd", dt, L=L, **AC))), outside=IN_REFUSALS),
    # acorr_bwd keeps the frame (rounded up to 8 bytes) and the M + 1 cotangents as doubles: with 3 lags the frame ends 6 (float32)
    # and 3 (float64) samples sooner -- between the two ceilings Autocorrelation has a forward and no gradient
    ceiling("csrc/lpc.hip::acorr_bwd_impl", "acorr_bwd: frame too long for LDS",
            inside=per(B32_64(15354, 7677), lambda dt, L: ("acorr_bwd", case("acorr", "bwd", dt, wrt=("x",), L=L, **AC))),
            outside=per(B32_64(15355, 7678), lambda dt, L: raises("acorr_bwd: frame too long for LDS", shape("acorr", "bwd", dt, wrt=("x",), L=L, **AC)))),
    # levdur_fwd_lds: 3 (M + 1) doubles.  The autocorrelation of white noise, frames four times the order, with the module's eps: the
    # float32 restatement stays at 1e-6 of the largest entry at these orders (MEASURED), so no better-conditioned input is needed
    ceiling("csrc/lpc.hip::levdur_fwd_impl", "levdur: order too large for LDS",
            inside=[("levdur_fwd_lds", case("levdur", "fwd", M=2559, **LD))], outside=IN_REFUSALS),
    # levdur_bwd_toeplitz: 7 M + 1 doubles
    ceiling("csrc/lpc.hip::levdur_bwd_impl", "levdur_bwd: order too large for LDS",
            inside=[("levdur_bwd_toeplitz", case("levdur", "bwd", wrt=("r",), M=1097, **LD))], outside=IN_REFUSALS),
    # frame_window_lpc_kernel: 4 frames of sizeof(T) L per block.  Past it fuse(Frame, Window, LPC) runs the three modules
    ceiling("csrc/lpc.hip::dsa_frame_window_lpc_fwd", "frame_window_lpc: frame too long for LDS",
            inside=per(B32_64(3840, 1920), lambda dt, L: ("frame_window_lpc_fwd", case("fwlpc", "fwd", dt, L=L, **FW))),
            outside=per(B32_64(3841, 1921), lambda dt, L: raises("frame_window_lpc: frame too long for LDS", shape("fwlpc", "fwd", dt, L=L, **FW)))
            + per(B32_64(3841, 1921), lambda dt, L: runs("levdur_fwd", case("fuse_fwlpc", "fwd", dt, L=L, **FW)))),
    # ---- csrc/spec.hip.  The direct row DFT keeps the row: sizeof(T) L <= 60 KB (fft_length 30: not a power of two)
    ceiling("csrc/spec.hip::launch_row_dft", E_ROW,
            inside=per(B32_64(15360, 7680), lambda dt, L: ("row_dft_generic", case("fftr", "fwd", dt, len_in=L, nfft=30, fmt=0, F=1))),
            outside=per(B32_64(15361, 7681), lambda dt, L: raises(E_ROW, shape("fftr", "fwd", dt, len_in=L, nfft=30, fmt=0, F=1)))),
    # its backward keeps 3 (fft_length / 2 + 1) values more: 48 samples sooner at fft_length 30 (a forward and no gradient between)
    ceiling("csrc/spec.hip::launch_row_dft_bwd", E_ROWB,
            inside=per(B32_64(15312, 7632), lambda dt, L: ("row_dft_bwd_generic", case("fftr", "bwd", dt, wrt=("x",), len_in=L, nfft=30, fmt=0, F=1))),
            outside=per(B32_64(15313, 7633), lambda dt, L: raises(E_ROWB, shape("fftr", "bwd", dt, wrt=("x",), len_in=L, nfft=30, fmt=0, F=1)))),
    # the FFT in LDS: sizeof(T) (L + 2 fft_length) <= 150 KB, with the raised LDS attribute.  At fft_length 4096 the row past it is
    # too long for the direct sum as well; float64 at 8192 (float32 at 16384) falls back to the direct sum 1 sample later, under the
    # other route name; a float64 row of 8192 samples at fft_length 8192 fits neither
    ceiling("csrc/spec.hip::launch_row_dft", "reshapes: the direct sum instead of the FFT in LDS, or " + E_ROW,
            inside=per(B32_64(30208, 11008), lambda dt, L: ("row_fft_generic", case("fftr", "fwd", dt, len_in=L, nfft=4096, fmt=0, F=1)))
            + [("row_fft_generic", case("fftr", "fwd", F64, len_in=2816, nfft=8192, fmt=0, F=1)),
               ("row_fft_generic", case("fftr", "fwd", F32, len_in=5632, nfft=16384, fmt=0, F=1))],
            outside=per(B32_64(30209, 11009), lambda dt, L: raises(E_ROW, shape("fftr", "fwd", dt, len_in=L, nfft=4096, fmt=0, F=1)))
            + [runs("row_dft_generic", case("fftr", "fwd", F64, len_in=2817, nfft=8192, fmt=0, F=1)),
               runs("row_dft_generic", case("fftr", "fwd", F32, len_in=5633, nfft=16384, fmt=0, F=1)),
               raises(E_ROW, shape("fftr", "fwd", F64, len_in=8192, nfft=8192, fmt=0, F=1))]),
    # its backward: sizeof(T) (L + 3 (fft_length / 2 + 1) + 2 fft_length) <= 150 KB, and the direct sum has no room either.  From
    # fft_length 8192 (float64) and 16384 (float32) on no row has a gradient at all, where the forward runs
    ceiling("csrc/spec.hip::launch_row_dft_bwd", "reshapes: the direct sum instead of the FFT in LDS, or " + E_ROWB,
            inside=per(B32_64(24061, 4861), lambda dt, L: ("row_fft_bwd_generic", case("fftr", "bwd", dt, wrt=("x",), len_in=L, nfft=4096, fmt=0, F=1))),
            outside=per(B32_64(24062, 4862), lambda dt, L: raises(E_ROWB, shape("fftr", "bwd", dt, wrt=("x",), len_in=L, nfft=4096, fmt=0, F=1)))
            + per(B32_64(16384, 8192), lambda dt, n: raises(E_ROWB, shape("fftr", "bwd", dt, wrt=("x",), len_in=16, nfft=n, fmt=0, F=1)))),
    # spec_ratio_bwd: sizeof(T) (lb + la + 5 (fft_length / 2 + 1)) <= 60 KB; the forward (two row transforms and spec_ratio) has the
    # row transform's ceilings only
    ceiling("csrc/spec.hip::dsa_spec_bwd", "spec_bwd: rows too long for LDS",
            inside=per(B32_64(6138, 3066), lambda dt, n: ("spec_ratio_bwd", case("spec", "bwd", dt, wrt=("b", "a"), nfft=n, **SR))),
            outside=per(B32_64(6140, 3068), lambda dt, n: raises("spec_bwd: rows too long for LDS", shape("spec", "bwd", dt, wrt=("b", "a"), nfft=n, **SR)))),
    # ---- csrc/fftcep.hip: more than 512 bins are refused in both dtypes and for every n_iter (float32 with n_iter = 0 has left the
    # matrix-core kernel at 320 bins).  The backward shares the launcher: its forward refuses first
    ceiling("csrc/fftcep.hip::fftcep_launch", "fftcep: fft_length above 1022 is not supported",
            inside=[("fftcep_fwd", case("fftcep", "fwd", nfft=1022, **a, **FFTCEP)) for a in (FC0, FC2)]
            + [("fftcep_bwd", case("fftcep", "bwd", wrt=("x",), nfft=1022, **a, **FFTCEP)) for a in (FC0, FC2)],
            outside=[raises("fftcep: fft_length above 1022 is not supported", shape("fftcep", "fwd", BOTH, nfft=1024, **a)) for a in (FC0, FC2)]),
    # ---- csrc/fbank.hip.  The generic kernels: 4 waves' tiles of 4 frames and the channel ranges in 150 KB --
    # 16 sizeof(T) K + 8 C forward, (16 sizeof(T) + 8) (K + C) backward (a forward and no gradient between)
    ceiling("csrc/fbank.hip::fbank_launch", E_FB,
            inside=per(B32_64(4778, 2388), lambda dt, n: ("fbank_fwd", case("fbank", "fwd", dt, nfft=n, **FB)))
            + per(B32_64(4104, 2096), lambda dt, n: ("fbank_bwd", case("fbank", "bwd", dt, wrt=("x",), nfft=n, **FB))),
            outside=per(B32_64(4780, 2390), lambda dt, n: raises(E_FB, shape("fbank", "fwd", dt, nfft=n, **FB)))
            + per(B32_64(4106, 2098), lambda dt, n: raises(E_FB, shape("fbank", "bwd", dt, wrt=("x",), nfft=n, **FB)))),
    # the filter matrix joins them in LDS while sizeof(T) K C more fits, else it stays in global memory (<T, false>: up to 16 waves
    # of tiles, above 64 KB at the ordinary fft_length 1024 / 80 channels with 64 frames)
    ceiling("csrc/fbank.hip::fbank_launch", "reshapes: the filter matrix stays in global memory",
            inside=per(B32_64(794, 396), lambda dt, n: ("fbank_fwd", case("fbank", "fwd", dt, nfft=n, **FB)))
            + per(B32_64(752, 364), lambda dt, n: ("fbank_bwd", case("fbank", "bwd", dt, wrt=("x",), nfft=n, **FB))),
            outside=per(B32_64(796, 398), lambda dt, n: runs("fbank_fwd", case("fbank", "fwd", dt, nfft=n, **FB)))
            + per(B32_64(754, 366), lambda dt, n: runs("fbank_bwd", case("fbank", "bwd", dt, wrt=("x",), nfft=n, **FB)))
            + [runs("fbank_fwd", case("fbank", "fwd", F32, nfft=1024, C=80, use_power=False, gamma=0.0, F=64)),
               runs("fbank_bwd", case("fbank", "bwd", F32, wrt=("x",), nfft=1024, C=80, use_power=False, gamma=0.0, F=64))]),
    # the matrix-core launcher takes float32 up to 320 bins and 48 channels (its LDS: 163 392 of 163 840 B at 320)
    ceiling("csrc/fbank.hip::dsa_fbank_fwd", "reshapes: the generic kernel instead of the matrix-core kernel",
            inside=[("fbank_mfma_fwd", case("fbank", "fwd", F32, nfft=638, C=12, use_power=False, gamma=0.0, F=5, **FBM))],
            outside=[runs("fbank_fwd", case("fbank", "fwd", F32, nfft=640, C=12, use_power=False, gamma=0.0, F=5))]),
    # MFCC: the second product costs the fused launch 3 KB more, so it ends at 309 bins; to 320 bins the two launches run
    ceiling("csrc/fbank.hip::dsa_fbank_dct_fwd", "reshapes: the filter bank and the DCT as two launches instead of one",
            inside=[("fbank_dct_mfma_fwd", case("mfcc", "fwd", F32, nfft=616, C=40, M=12, F=7, **MFCC))],
            outside=[runs("freqt_lds_fwd", case("mfcc", "fwd", F32, nfft=618, C=40, M=12, F=7, **MFCC))]),
    # ---- csrc/plp.hip
    plp_waves("2 waves per block instead of 4", 3538, 1704),
    plp_waves("1 wave per block instead of 2", 7634, 3752),
    # one wave's slice against 160 KB, with the raised attribute above 64 KB; the backward has the forward's geometry
    ceiling(("csrc/plp.hip::plp_launch_fwd", "csrc/plp.hip::plp_launch_bwd"), E_PLP,
            inside=per(B32_64(40402, 20136), lambda dt, n: ("plp_fwd", case("plp_tail", "fwd", dt, n_fft=n, **PL, **PLP_OUT)))
            + per(B32_64(40402, 20136), lambda dt, n: ("plp_bwd", case("plp_tail", "bwd", dt, wrt=("y", "E"), n_fft=n, **PL))),
            outside=per(B32_64(40404, 20138), lambda dt, n: raises(E_PLP, shape("plp_tail", "fwd", dt, n_fft=n, **PL))),
            shadowed=(E_PLPB,)),
    # ---- csrc/mlsacheck.hip (fast: one bin; scale and clip: fft_length / 2 + 1 bins at cep_order 24)
    mlsa_rows("fast", 9214, 6142, 1, "M"),
    mlsa_rows("scale", 18380, 18354, 2, "n_fft"),
    mlsa_rows("clip", 18380, 18354, 2, "n_fft"),
    # ---- csrc/zerodf.hip: what is still refused behind the tap pieces (ZDF_PIECES holds the accepted side of those): a filter too
    # long for one launch with ignore_gain or a frame period that is no multiple of 4 -- 3 M + 2 + P values against 64 KB
    ceiling("csrc/zerodf.hip::zerodf_launch_fwd", "zerodf: filter too long for LDS",
            inside=per(B32_64(5459, 2729), lambda dt, M: ("zerodf_fwd", case("zerodf", "fwd", dt, M=M, **ZF, **ZDF_FWD))),
            outside=per(B32_64(5460, 2730), lambda dt, M: raises("zerodf: filter too long for LDS", shape("zerodf", "fwd", dt, M=M, **ZF))),
            cited=ZDF_PIECES),
    # the tap gradient of the first kernels: 4 P + M + 256 values against 64 KB, which binds before the forward only at frame periods
    # from 1421 (float64) and 2911 (float32) on
    ceiling("csrc/zerodf.hip::zerodf_launch_bwd", "zerodf_bwd: filter too long for LDS",
            inside=[("zerodf_bwd", case("zerodf", "bwd", F32, wrt=("x", "b"), M=4484, P=2911, **ZB, **ZDF_BWD)),
                    ("zerodf_bwd", case("zerodf", "bwd", F64, wrt=("x", "b"), M=2252, P=1421, **ZB, **ZDF_BWD))],
            outside=[raises("zerodf_bwd: filter too long for LDS", shape("zerodf", "bwd", F32, wrt=("x", "b"), M=4485, P=2911, **ZB)),
                     raises("zerodf_bwd: filter too long for LDS", shape("zerodf", "bwd", F64, wrt=("x", "b"), M=2253, P=1421, **ZB))],
            cited=ZDF_PIECES),
    # ---- csrc/mgc.hip, at the entries themselves (ops.gc2gc_fused / gc2gc_fn test the same sizes first and hand longer transforms to
    # the operator chain).  Forward: 2 sizeof(T) n_fft <= 150 KB; backward: 5 sizeof(T) n_fft / 2 + 64 -- one power of two sooner
    ceiling("csrc/mgc.hip::dsa_gc2gc_fwd", E_GC,
            inside=per(B32_64(16384, 8192), lambda dt, n: ("gc2gc_fused", case("gc2gc_entry", "fwd", dt, n_fft=n, **GE, **GCF))),
            outside=per(B32_64(32768, 16384), lambda dt, n: raises(E_GC, shape("gc2gc_entry", "fwd", dt, n_fft=n, **GE)))),
    ceiling("csrc/mgc.hip::dsa_gc2gc_bwd", E_GCB,
            inside=per(B32_64(8192, 4096), lambda dt, n: ("gc2gc_fused_bwd", case("gc2gc_entry", "bwd", dt, wrt=("c",), n_fft=n, **GE, **GC))),
            outside=per(B32_64(16384, 8192), lambda dt, n: raises(E_GCB, shape("gc2gc_entry", "bwd", dt, wrt=("c",), n_fft=n, **GE)))),
    # (more than 2^31 - 1 rows share the message)
    ceiling("csrc/mgc.hip::dsa_gc2gc_fwd", "gc2gc: out_order + 1 must not exceed n_fft",
            inside=[("gc2gc_fused", case("gc2gc_entry", "fwd", g1=-0.5, g2=0.0, n_fft=4, m1=2, m2=3, F=2, **GCF))],
            outside=[raises("gc2gc: out_order + 1 must not exceed n_fft", shape("gc2gc_entry", "fwd", BOTH, g1=-0.5, g2=0.0, n_fft=4, m1=2, m2=4, F=2))]),
    ceiling("csrc/mgc.hip::dsa_mgcep_spectra", "mgcep_spectra: cep_order above 64",
            inside=[("mgcep_spectra", case("mgcep_spectra", "fwd", nfft=256, M=64, gamma=-0.5, F=3))],
            outside=[raises("mgcep_spectra: cep_order above 64", shape("mgcep_spectra", "fwd", BOTH, nfft=256, M=65, gamma=-0.5, F=3))]),
    # ---- csrc/mcep.hip, the generic pair (asked for by name: float32 geometries of this size go to the whole-batch composition):
    # sizeof(T) (3 K + M1^2 + 7 M1 - 1) <= 160 KB, the attribute set on every launch.  The backward has the forward's size
    ceiling(("csrc/mcep.hip::mcep_generic_fwd", "csrc/mcep.hip::mcep_generic_bwd"), "mcep: configuration exceeds LDS",
            inside=per(B32_64(27208, 13556), lambda dt, n: ("mcep_generic_fwd", case("mcep_generic", "fwd", dt, nfft=n, **MG)))
            + per(B32_64(27208, 13556), lambda dt, n: ("mcep_generic_bwd", case("mcep_generic", "bwd", dt, wrt=("X",), nfft=n, **MG))),
            outside=per(B32_64(27210, 13558), lambda dt, n: raises("mcep: configuration exceeds LDS", shape("mcep_generic", "fwd", dt, nfft=n, **MG)))),
    # ---- csrc/mdct.hip: the fast kernels end at frame length 4096 (48 KB of LDS in the synthesis: no attribute needed)
    ceiling("csrc/mdct.hip::md_check", "reshapes: the generic kernels instead of the fast ones",
            inside=[("mdct_analysis_fast", case("mdct", "fwd", F32, L=4096, T=5000, B=1)), ("mdct_synthesis_fast", case("imdct", "fwd", F32, L=4096, N=3, B=1))],
            outside=[runs("mdct_analysis_generic", case("mdct", "fwd", F32, L=8192, T=9000, B=1)),
                     runs("mdct_synthesis_generic", case("imdct", "fwd", F32, L=8192, N=3, B=1))]),
]

# launches above 48 KB of dynamic LDS whose size does not depend on the call, so every test of the route runs the largest shape
LDS_FIXED = {
    "poledf_ring_fwd": "tests/test_gpu_poledf.py::test_ring_kernels_are_the_ones_that_run",
    "poledf_ring_bwd": "tests/test_gpu_poledf.py::test_ring_kernels_are_the_ones_that_run",
    "lsp_lpc2lsp_fwd": "tests/test_gpu_lsp.py::test_tile_and_dispatch_edges",
    "th_solve_quadn_fwd": "tests/test_gpu_synth.py::test_thsolve_kernel_vs_numpy_and_gradcheck",   # (41 984 B at most: below the attribute)
}

# ---- every other DSA_ERR_UNSUPPORTED of csrc/: message (as the source spells it, without the trailing %s) -> why no size a caller
# can reach meets it.  tests/test_routes_cpu.py holds the three tables against the sources.
DTYPE = "ops._core._dtype_code raises TypeError for anything but float32 / float64 before the entry is called"
NOT_A_CEILING = {
    # with_dtype of csrc/common.h, which speaks every entry's dtype refusal under the entry's name (tests/test_dtype_refusals_cpu.py calls each)
    "%s: unsupported dtype": DTYPE,
    "fbank_bins_bwd: float32 only (the fused forward it differentiates is)": "ops.StftFbankFn is the only caller and FusedSTFTFilterBank._fusable "
        "admits float32 only",
    "mcep_newton_update: float32 only": "ops.mcep._mcep_composed_applies admits float32 only",
    "mcep_newton_update_bwd: float32 only": "the backward of ops.McepNewtonUpdateFn, whose forward is float32 (_mcep_composed_applies)",
    "rows_gemm: float32 only": "ops.rows callers come from _mcep_composed_applies: float32 only",
    "rows_ew: float32 only": "ops.rows.RowsLogFn / RowsExpSubFn are used by the float32 composition only (_mcep_composed_applies)",
    "mcep_newton_steps: float32 only": "ops.mcep.mcep_newton_steps is reached from the float32 composition only",
    "mcep_newton_resid_h_bwd: float32 only": "as mcep_newton_steps: the float32 composition only",
    "mcep_newton_glogx_h: float32 only": "as mcep_newton_steps: the float32 composition only",
    # the tuned entries: the caller tests the geometry before it calls
    "stft: tuned kernel needs float32, fft_length 512, frame_length <= 512": "only with DSA_ALGO_TUNED asked for by name; ops.StftFn passes "
        "ALGO_AUTO, which falls back to the generic route",
    "stft_bwd: tuned kernel needs float32, fft_length 512, constant padding, no floor, fixed window": "as the forward: DSA_ALGO_TUNED by name only",
    "stft_fbank: the fused kernel needs float32, fft_length 512, frame_length 400, an even frame period and at most 126 channels "
    "(use dsa_stft_fwd + dsa_fbank_fwd)": "modules.fused.FusedSTFTFilterBank._fusable tests the same geometry first and runs the two modules otherwise",
    "mcep: tuned kernel needs float32, fft_length 512, cep_order 24": "DSA_ALGO_TUNED by name only; the module passes ALGO_AUTO or ALGO_GENERIC",
    "mcep_bwd: tuned kernel needs float32, fft_length 512, cep_order 24": "as the forward: DSA_ALGO_TUNED by name only",
    "stft_mcep: the fused launch covers float32, frame_length 400, fft_length 512, cep_order 24": "modules.fused.FusedSTFTMelCepstralAnalysis "
        "tests ops.stft_mcep_fusable first and runs the two stages otherwise",
    "mgcep_step: needs float32, fft_length 512, cep_order <= 24": "modules.mgcep builds the step images only for that geometry and calls "
        "ops.mgcep_step only with them",
    "mgcep_step_bwd: needs float32, fft_length 512, cep_order <= 24": "the backward of ops.MgcepStepFn: same geometry as its forward",
    "mgcep_step_bwd_h: needs float32, fft_length 512, cep_order 24": "ops.mgc._step_bwd_entry picks it from the binary16 images, which "
        "modules.mgcep builds at cep_order 24 only",
    "mgcep_step_solve: needs float32, fft_length 512, cep_order 24": "modules.mgcep calls it with the order-24 images only",
    "thsolve_update: order 24 in float32 only (dsa_thsolve_fwd + an addition otherwise)": "ops.mgc.thsolve_update returns None for any "
        "other order or dtype and the caller adds the solution itself",
    "frame_window_lpc_bwd: the one-launch backward covers float32, lpc_order 24, 25 <= frame_length <= 512, constant padding":
        "ops.frame_window_lpc_bwd_supported restates the launcher's conditions; FusedFrameWindowLPC asks it first",
    "frame_window_lpc_bwd: frame_length + frame_period above 1024": "ops.frame_window_lpc_bwd_supported (L + P <= 1024)",
    "frame_window_lpc_bwd: this frame_length / frame_period pair does not fit the one-launch backward": "ops.frame_window_lpc_bwd_supported (the halo test)",
    "%s: the fast kernels take float32 and a power-of-two frame length in their range": "DSA_ALGO_TUNED by name only; ops.mdct passes "
        "ALGO_AUTO, which takes the generic kernels (the CEILINGS row of csrc/mdct.hip::md_check holds that edge)",
    "fbank: spectrum too long for the matrix-core kernel's LDS": "every caller of fbank_mfma_launch_ex tests K <= 320 first (dsa_fbank_fwd, "
        "dsa_freqt_fwd, dsa_fftcep_fwd: 163 392 B at 320), and dsa_fbank_dct_fwd tests fbank_mfma_lds_bytes(K, true) itself",
    # orders and plans: dispatch inside the library, or properties of a matrix rather than a size
    "thsolve_quad: order below 2": "dsa_thsolve_fwd and dsa_mcep_newton_update send order 1 to the one-wave kernel",
    "thsolve_quad: order above 55": "dsa_thsolve_fwd sends orders above 55 to the one-wave kernel; the composition ends at order 54 + 1",
    "mcep_resid: order above 55": "ops.mcep._mcep_composed_fwd uses two dsa_rows_gemm launches above order 54",
    "mcep_newton_resid: float32, orders up to 54": "as mcep_resid: the caller's own order test",
    "mcep_resid_prepare: float32, orders up to 54": "ops.mcep.mcep_resid_images returns None above order 54",
    "mcep_newton_resid_h: float32, orders up to 54": "called with the images of mcep_resid_images only",
    "mcep_newton_steps: no one-launch kernel for this order (32 .. 54)": "ops.mcep.mcep_newton_steps_applies tests the order; ERR_UNSUPPORTED "
        "makes the caller alternate the two launches",
    "mcep_resid_bwd_prepare: float32, orders 32 .. 54": "ops.mcep.mcep_resid_bwd_images asks dsa_mcep_resid_bwd_images_bytes first (0: composed gradient)",
    "mcep_newton_resid_h_bwd: orders 32 .. 54": "called with the images of mcep_resid_bwd_images only",
    "rows_gemm: unsupported combination of flags": "ops.rows passes the three combinations the switch has",
    "rows_ew: unknown operation": "ops.rows passes operation 0 or 1",
    "zerodf: the scaled / accumulating form needs P % 4 == 0 and M >= 16": "ops.filters.zerodf_taylor is used only where "
        "ops.filters.zerodf_taylor_shapes_ok (the same test) holds",
    "zerodf_bwd: the scaled / accumulating form needs P % 4 == 0 and M >= 16": "as its forward",
    "fbank_bins_plan: non-finite matrix": "a property of the matrix, not a size: ops.fbank_bins_table keeps the dense backward then",
    "fbank_bins_plan: a bin feeds more than two adjacent channels": "a property of the matrix: ops.fbank_bins_table keeps the dense backward",
    "fbank_scan_plan: needs 257 bins and at most 126 channels": "ops.fbank_scan_plan tests both before it calls",
    "fbank_scan_plan: non-finite weight": "a property of the matrix: ops.fbank_scan_plan returns None and the two modules run",
    "fbank_scan_plan: channels are not ordered along the bins": "a property of the matrix: the two modules run",
    "fbank_scan_plan: a bin feeds more than two adjacent channels": "a property of the matrix: the two modules run",
    # more than 2^31 rows
    "frame_bwd: batch too large for one launch": "more than 2^31 - 1 blocks of 256 threads: beyond any tensor the tests or a device can hold",
    # without a message: the caller keeps the composed path
    "return DSA_ERR_UNSUPPORTED @ mcep_big.hip x2": "dsa_mcep_newton_steps turns it into its own message (above); orders outside 32 .. 54",
    "return DSA_ERR_UNSUPPORTED @ mcep_resid.hip x3": "dsa_mcep_newton_resid_h_bwd / _glogx_h: orders outside 32 .. 54 or more steps than one "
        "workgroup's LDS holds; ops.mcep keeps the composed gradient",
}


def all_cases():
    """(route, case) of everything that is compared: ROUTES, and both sides of CEILINGS"""
    out = [(route, c) for route, cases in ROUTES.items() for c in cases]
    for row in CEILINGS:
        out += list(row["inside"])
        if row["outside"] != IN_REFUSALS:
            out += [(o["route"], o["case"]) for o in row["outside"] if o["expect"] == "route"]
    return out


PINNED_ELSEWHERE = {
    "delta_fwd": "tests/test_gpu_paramgen.py::test_delta_against_the_goldens",
    "div_rows": "tests/test_gpu_istft.py::test_unframe_matches_oracle_and_autograd",
    "excite_f32": "tests/test_gpu_excite.py::test_against_the_reference",
    "excite_f64": "tests/test_gpu_excite.py::test_against_the_reference",
    "fbank_fwd": "tests/test_gpu_parity.py::test_fbank_mfcc_golden_forward_backward",
    "fbank_mfma_fwd": "tests/test_gpu_parity.py::test_fbank_mfcc_golden_forward_backward",
    "fbank_dct_mfma_fwd": "tests/test_gpu_parity.py::test_fbank_mfcc_golden_forward_backward",
    "fftcep_fwd": "tests/test_gpu_parity.py::test_fftcep_golden_forward_backward",
    "fftcep_fft_fwd": "tests/test_gpu_parity.py::test_fftcep_golden_forward_backward",
    "fftcep_mfma_fwd": "tests/test_gpu_parity.py::test_fftcep_golden_forward_backward",
    "frame_fwd": "tests/test_gpu_alignment.py::test_frame_forward",
    "frame_fwd_vec4": "tests/test_gpu_alignment.py::test_frame_forward",
    "frame_bwd": "tests/test_gpu_alignment.py::test_stft_big_backward",
    "window_fwd": "tests/test_gpu_alignment.py::test_window_forward_and_backward",
    "window_vec4": "tests/test_gpu_alignment.py::test_window_forward_and_backward",
    "window_bwd": "tests/test_gpu_alignment.py::test_window_forward_and_backward",
    "stft512_fwd": "tests/test_gpu_alignment.py::test_stft512_forward_and_backward",
    "stft512_bwd": "tests/test_gpu_parity.py::test_griffin_lim_golden",
    "stft512_bwd_pk": "tests/test_gpu_parity.py::test_stft_istft_round_trip",
    "stft512_fbank_fwd": "tests/test_gpu_alignment.py::test_fused_stft_fbank",
    "stft512_mcep_fused_fwd": "tests/test_gpu_alignment.py::test_fused_stft_mcep",
    "stft1024_fwd": "tests/test_gpu_stft_big.py::test_bench_size_properties_parseval_and_partition_invariance",   # f"stft{nfft}_fwd"
    "stft2048_fwd": "tests/test_gpu_stft_big.py::test_bench_size_properties_parseval_and_partition_invariance",
    "stft1024_bwd": "tests/test_gpu_alignment.py::test_stft_big_backward",                                         # f"stft{nfft}_bwd"
    "stft2048_bwd": "tests/test_gpu_alignment.py::test_stft_big_backward",
    "griffin_update": "tests/test_gpu_parity.py::test_griffin_lim_full_size_properties",
    "lpc24_bwd": "tests/test_gpu_alignment.py::test_lpc24_backward",
    "frame_window_lpc24_mfma_fwd": "tests/test_gpu_lpc_fused.py::test_fused_lpc_golden_forward_and_gradient",
    "frame_window_lpc24_bwd_mfma": "tests/test_gpu_alignment.py::test_fused_lpc_forward_and_backward",
    "gc2gc_fused": "tests/test_gpu_synth.py::test_gc2gc_fused_kernel_equals_the_operator_chain",
    "gnorm_fwd": "tests/test_gpu_synth.py::test_gain_normalisation_kernels_against_the_stock_composition",
    "ignorm_fwd": "tests/test_gpu_synth.py::test_gain_normalisation_kernels_against_the_stock_composition",
    "mgcep_step_solve": "tests/test_gpu_configs.py::test_mgcep_whole_step_in_one_launch_against_the_two_launch_step_and_the_oracle",
    "mgcep_step_bwd_h": "tests/test_gpu_configs.py::test_mgcep_step_adjoint_on_binary16_splits_against_the_float32_kernel",
    "th_solve_fwd": "tests/test_gpu_synth.py::test_thsolve_kernel_vs_numpy_and_gradcheck",
    "th_solve_quad_fwd": "tests/test_gpu_synth.py::test_thsolve_kernel_vs_numpy_and_gradcheck",
    "th_solve_quadn_fwd": "tests/test_gpu_synth.py::test_thsolve_kernel_vs_numpy_and_gradcheck",
    "th_solve_octn_fwd": "tests/test_gpu_configs.py::test_untuned_geometries_forward_as_whole_batch_launches",
    "mcep_big_newton": "tests/test_gpu_configs.py::test_untuned_geometries_forward_as_whole_batch_launches",
    "mcep_generic_fwd": "tests/test_gpu_configs.py::test_untuned_geometries_forward_as_whole_batch_launches",
    "mcep_mfma_fwd": "tests/test_gpu_configs.py::test_config5_shard_1024_utterances",
    "mcep_resid_h": "tests/test_gpu_configs.py::test_newton_residual_on_binary16_splits_against_float64",
    "mcep_resid_mfma": "tests/test_gpu_configs.py::test_newton_residual_in_one_launch_against_float64",
    "mcep_resid_bwd_h": "tests/test_gpu_48k_grad.py::test_resid_h_bwd_entry_vs_float64_autograd_of_its_formula",
    "rows_gemm_mfma": "tests/test_gpu_configs.py::test_rows_gemm_matrix_core_product_against_float64",
    "rows_gemm_mfma_t": "tests/test_gpu_configs.py::test_rows_gemm_matrix_core_product_against_float64",
    "mcpf_fwd": "tests/test_gpu_paramgen.py::test_mcpf_against_the_goldens",
    "mcpf_bwd": "tests/test_gpu_paramgen.py::test_mcpf_gradcheck",
    "mlpg_forward_reg": "tests/test_gpu_paramgen.py::test_mlpg_against_the_goldens",
    "mlpg_forward_any": "tests/test_gpu_paramgen.py::test_mlpg_against_the_goldens",
    "mlpg_adjoint_reg": "tests/test_gpu_paramgen.py::test_element_aligned_operands_views_and_empty_batches",
    "poledf_ring_fwd": "tests/test_gpu_poledf.py::test_ring_kernels_are_the_ones_that_run",
    "poledf_ring_bwd": "tests/test_gpu_poledf.py::test_ring_kernels_are_the_ones_that_run",
    "poledf_bwd_a": "tests/test_gpu_poledf.py::test_ring_kernels_are_the_ones_that_run",
    "poledf_generic_fwd": "tests/test_gpu_poledf.py::test_generic_path_against_the_oracle",
    "pqmf_fwd_generic": "tests/test_gpu_pqmf.py::test_tuned_and_generic_kernels_are_the_ones_that_run",
    "pqmf_fwd_tuned": "tests/test_gpu_pqmf.py::test_tuned_and_generic_kernels_are_the_ones_that_run",     # f"pqmf_fwd_{want}"
    "ipqmf_fwd_tuned": "tests/test_gpu_pqmf.py::test_tuned_and_generic_kernels_are_the_ones_that_run",    # f"ipqmf_fwd_{want}"
    "ipqmf_fwd_generic": "tests/test_gpu_pqmf.py::test_tuned_and_generic_kernels_are_the_ones_that_run",
    # f"lsp_{name}_fwd" / f"lsp_{name}_bwd", name in lpc2lsp, lsp2lpc, lspcheck
    **{f"lsp_{n}_{d}": "tests/test_gpu_lsp.py::test_tile_and_dispatch_edges" for n in ("lpc2lsp", "lsp2lpc", "lspcheck") for d in ("fwd", "bwd")},
    # family + name + "_fwd" / "_bwd", family parcor_lane_ up to order 63 and parcor_row_ above
    **{f"parcor_{f}_{n}_{d}": "tests/test_gpu_parcor.py::test_tile_and_dispatch_edges"
       for f in ("lane", "row") for n in ("lpc2par", "par2lpc", "lpccheck") for d in ("fwd", "bwd")},
    # kernel_name(dtype, M, mode, n_fft, bwd): f"mlsacheck_{tuned or generic}_{fwd or bwd}", both sides of the boundary asserted reached
    **{f"mlsacheck_{k}_{d}": "tests/test_gpu_mlsacheck.py::test_tile_and_dispatch_edges" for k in ("tuned", "generic") for d in ("fwd", "bwd")},
    # ---- the families whose launchers index a name table by entry, route and dtype; each pointer is the test that compares the entry
    # with its reference and the list of its launches' names with these
    # kDtwRoutes (csrc/dtw.hip): one wave up to 64 rows, a workgroup beyond; the path's kernel is the same on both
    **{f"dtw_{e}{r}_{d}": "tests/test_gpu_dtw.py::test_golden_parity_paths_and_routes" for e in ("", "vjp_") for r in ("wave", "block") for d in BOTH},
    **{f"dtw_path_{d}": "tests/test_gpu_dtw.py::test_golden_parity_paths_and_routes" for d in BOTH},
    # kGmmRoutes (csrc/gmm.hip): the four launches of an EM iteration on the full and the diagonal route; regress and transform have one
    **{f"gmm_{e}_{r}_{d}": "tests/test_gpu_gmm.py::test_golden_parity_and_routes"
       for e in ("prepare", "estep", "accum", "update") for r in ("full", "diag") for d in BOTH},
    **{f"gmm_{e}_{d}": "tests/test_gpu_gmm.py::test_transform_on_the_goldens" for e in ("regress", "transform") for d in BOTH},
    # kYinRoutes (csrc/yingram.hip): both routes asked for by name
    **{f"yingram_{e}{r}_{d}": "tests/test_gpu_yingram.py::test_golden_parity_and_routes" for e in ("", "vjp_") for r in ("direct", "fft") for d in BOTH},
    **{f"frame_yingram_{r}_{d}": "tests/test_gpu_yingram.py::test_fused_equals_the_two_modules" for r in ("direct", "fft") for d in BOTH},
    # kVqRoutes (csrc/vq.hip): the update works on float64 partial sums whatever the dtype of x
    **{f"vq_{e}_{d}": "tests/test_gpu_lbg.py::test_vq_and_ivq_match_a_float64_composition" for e in ("search", "lookup") for d in BOTH},
    **{f"vq_accum_{d}": "tests/test_gpu_lbg.py::test_counts_and_centroids_are_exact" for d in BOTH},
    "vq_update": "tests/test_gpu_lbg.py::test_counts_and_centroids_are_exact",
    **{f"vq_vjp_{d}": "tests/test_gpu_lbg.py::test_training_mode_loss_and_gradient" for d in BOTH},
    # kWsRoutes (csrc/world_synth.hip): the module's forward ends in the overlap-add, and its backward runs on autograd's thread, so the
    # launches between are called one by one
    **{f"world_synth_pulses_{d}": "tests/test_gpu_world_synth.py::test_pulse_lists_are_the_references" for d in BOTH},
    **{f"world_synth_overlap_add_{d}": "tests/test_gpu_world_synth.py::test_parity_with_the_reference" for d in BOTH},
    **{f"world_synth_{e}_{d}": "tests/test_gpu_world_synth.py::test_every_launch_names_its_kernel" for e in ("responses", "vjp_pulses", "vjp_frames") for d in BOTH},
    # kApRoutes (csrc/ap.hip): as WorldSynthesis -- the forward ends in the tandem kernel
    **{f"ap_tandem_{d}": "tests/test_gpu_ap.py::test_parity_with_the_reference" for d in BOTH},
    **{f"ap_{e}_{d}": "tests/test_gpu_ap.py::test_every_launch_names_its_kernel" for e in ("qmf", "qmf_vjp", "tandem_vjp") for d in BOTH},
    # csrc/pitch_spec.hip keeps no table: each entry picks its pair into a local and hands it to ps_launch (FORWARDED below).  The backward
    # runs on autograd's thread, so the test calls the three entries one by one
    **{f"pitch_spec{e}_{d}": "tests/test_gpu_pitch_spec.py::test_every_launch_names_its_kernel" for e in ("", "_vjp_frames", "_vjp_gather") for d in BOTH},
}

# names passed to a shared launcher as an argument, or kept in a local before the call: name -> "csrc/<file>::<function that spells it>"
FORWARDED = {
    "mlsacheck_generic_fwd": "csrc/mlsacheck.hip::mlsacheck_generic_launch", "mlsacheck_generic_bwd": "csrc/mlsacheck.hip::mlsacheck_generic_launch",
    "fbank_mfma_fwd": "csrc/fbank.hip::fbank_mfma_launch", "fbank_dct_mfma_fwd": "csrc/fbank.hip::dsa_fbank_dct_fwd", "freqt_mfma_fwd": "csrc/mcep.hip::dsa_freqt_fwd",
    "fftcep_mfma_fwd": "csrc/fftcep.hip::dsa_fftcep_fwd",
    **{f"pitch_spec{e}_{d}": f"csrc/pitch_spec.hip::dsa_pitch_spec{e}" for e in ("", "_vjp_frames", "_vjp_gather") for d in BOTH},
}

EXEMPT = {
    "pqmf_bwd_f": "dsa_pqmf_bwd launches pqmf_f_sum right behind it, so last_kernel() never shows it; its partial sums are the filter "
                  "gradient that the pqmf_f_sum case compares with float64",
    "ipqmf_bwd_f": "dsa_ipqmf_bwd launches pqmf_f_sum right behind it, so last_kernel() never shows it; its partial sums are the filter "
                   "gradient that the pqmf_f_sum case (ipqmf) compares with float64",
    "mcep_prepare": "packs G, D, E into the binary16 operand images of the tuned kernels, an internal layout with no definition of its own: "
                    "a wrong image fails tests/test_gpu_configs.py::test_config3_backward_batch256_vs_float64_autograd",
    "mcep_resid_prepare": "packs D, E into the residual kernel's binary16 images (internal layout): a wrong image fails "
                          "tests/test_gpu_configs.py::test_newton_residual_on_binary16_splits_against_float64",
    "mcep_resid_bwd_prepare": "packs D, E into the residual adjoint's binary16 images (internal layout): a wrong image fails "
                              "tests/test_gpu_48k_grad.py::test_resid_h_bwd_entry_vs_float64_autograd_of_its_formula",
}

# case id -> (base64, base32), printed by `python tests/routes_ref.py`
MEASURED = {
    "levdur_fwd-levdur-fwd-M0-eps0.0": (0.00e+00, 1.51e-08),
    "levdur_fwd-levdur-fwd-M0-eps1e-05": (0.00e+00, 1.51e-08),
    "levdur_fwd-levdur-fwd-M1-eps0.0": (0.00e+00, 2.79e-08),
    "levdur_fwd-levdur-fwd-M1-eps1e-05": (0.00e+00, 3.64e-08),
    "levdur_fwd-levdur-fwd-M62-eps0.0": (5.44e-18, 3.33e-08),
    "levdur_fwd-levdur-fwd-M62-eps1e-05": (7.25e-18, 2.84e-08),
    "levdur_fwd-levdur-fwd-M63-eps0.0": (8.70e-18, 2.24e-08),
    "levdur_fwd-levdur-fwd-M63-eps1e-05": (1.11e-16, 1.84e-08),
    "levdur_fwd_lds-levdur-fwd-M64-eps0.0": (1.03e-17, 4.71e-08),
    "levdur_fwd_lds-levdur-fwd-M64-eps1e-05": (1.12e-17, 3.81e-08),
    "levdur_fwd_lds-levdur-fwd-M65-eps0.0": (6.25e-18, 1.73e-08),
    "levdur_fwd_lds-levdur-fwd-M65-eps1e-05": (1.14e-16, 2.28e-08),
    "levdur_fwd_lds-levdur-fwd-M100-eps0.0": (1.82e-16, 3.43e-08),
    "levdur_fwd_lds-levdur-fwd-M100-eps1e-05": (7.81e-18, 3.64e-08),
    "levdur_fwd_lds-lpc-fwd-L404-M100-eps1e-05": (6.50e-18, 6.18e-08),
    "levdur_bwd-levdur-bwd-M1-eps1e-05": (0.00e+00, 1.07e-07),
    "levdur_bwd-levdur-bwd-M24-eps1e-05": (3.61e-16, 1.10e-07),
    "levdur_bwd-levdur-bwd-M63-eps1e-05": (5.40e-16, 1.92e-07),
    "levdur_bwd-levdur-bwd-M64-eps1e-05": (5.16e-16, 1.54e-07),
    "levdur_bwd-levdur-bwd-M85-eps1e-05": (8.04e-16, 2.49e-07),
    "levdur_bwd_toeplitz-levdur-bwd-M86-eps1e-05": (4.89e-16, 2.64e-07),
    "levdur_bwd_toeplitz-levdur-bwd-M100-eps1e-05": (4.82e-16, 1.29e-07),
    "acorr_fwd-acorr-fwd-L1-M0-fmt0": (0.00e+00, 4.11e-08),
    "acorr_fwd-acorr-fwd-L1-M0-fmt1": (0.00e+00, 0.00e+00),
    "acorr_fwd-acorr-fwd-L1-M0-fmt2": (0.00e+00, 2.89e-08),
    "acorr_fwd-acorr-fwd-L1-M0-fmt3": (0.00e+00, 9.60e-09),
    "acorr_fwd-acorr-fwd-L63-M0-fmt0": (0.00e+00, 6.64e-08),
    "acorr_fwd-acorr-fwd-L63-M0-fmt1": (0.00e+00, 0.00e+00),
    "acorr_fwd-acorr-fwd-L63-M0-fmt2": (1.73e-16, 1.24e-07),
    "acorr_fwd-acorr-fwd-L63-M0-fmt3": (2.03e-16, 5.10e-08),
    "acorr_fwd-acorr-fwd-L63-M7-fmt0": (1.12e-16, 9.67e-08),
    "acorr_fwd-acorr-fwd-L63-M7-fmt1": (5.55e-17, 2.67e-08),
    "acorr_fwd-acorr-fwd-L63-M7-fmt2": (1.02e-16, 3.01e-08),
    "acorr_fwd-acorr-fwd-L63-M7-fmt3": (1.99e-16, 8.54e-08),
    "acorr_fwd-acorr-fwd-L63-M62-fmt0": (1.11e-16, 1.11e-07),
    "acorr_fwd-acorr-fwd-L63-M62-fmt1": (1.11e-16, 3.56e-08),
    "acorr_fwd-acorr-fwd-L63-M62-fmt2": (5.20e-17, 6.38e-08),
    "acorr_fwd-acorr-fwd-L63-M62-fmt3": (2.03e-16, 1.38e-07),
    "acorr_fwd-acorr-fwd-L64-M0-fmt0": (0.00e+00, 5.78e-08),
    "acorr_fwd-acorr-fwd-L64-M0-fmt1": (0.00e+00, 0.00e+00),
    "acorr_fwd-acorr-fwd-L64-M0-fmt2": (2.12e-16, 1.53e-08),
    "acorr_fwd-acorr-fwd-L64-M0-fmt3": (0.00e+00, 1.37e-07),
    "acorr_fwd-acorr-fwd-L64-M7-fmt0": (2.08e-16, 4.13e-08),
    "acorr_fwd-acorr-fwd-L64-M7-fmt1": (5.55e-17, 3.33e-08),
    "acorr_fwd-acorr-fwd-L64-M7-fmt2": (1.08e-16, 3.12e-08),
    "acorr_fwd-acorr-fwd-L64-M7-fmt3": (5.20e-17, 7.30e-08),
    "acorr_fwd-acorr-fwd-L64-M63-fmt0": (7.03e-17, 4.64e-08),
    "acorr_fwd-acorr-fwd-L64-M63-fmt1": (8.33e-17, 3.42e-08),
    "acorr_fwd-acorr-fwd-L64-M63-fmt2": (2.13e-16, 2.77e-08),
    "acorr_fwd-acorr-fwd-L64-M63-fmt3": (7.90e-17, 5.85e-08),
    "acorr_fwd-acorr-fwd-L65-M0-fmt0": (0.00e+00, 4.79e-08),
    "acorr_fwd-acorr-fwd-L65-M0-fmt1": (0.00e+00, 0.00e+00),
    "acorr_fwd-acorr-fwd-L65-M0-fmt2": (1.66e-16, 7.61e-08),
    "acorr_fwd-acorr-fwd-L65-M0-fmt3": (0.00e+00, 9.85e-08),
    "acorr_fwd-acorr-fwd-L65-M7-fmt0": (1.67e-16, 3.17e-08),
    "acorr_fwd-acorr-fwd-L65-M7-fmt1": (4.16e-17, 2.74e-08),
    "acorr_fwd-acorr-fwd-L65-M7-fmt2": (1.89e-16, 8.89e-08),
    "acorr_fwd-acorr-fwd-L65-M7-fmt3": (4.90e-17, 7.02e-08),
    "acorr_fwd-acorr-fwd-L65-M64-fmt0": (1.05e-16, 6.11e-08),
    "acorr_fwd-acorr-fwd-L65-M64-fmt1": (5.55e-17, 4.40e-08),
    "acorr_fwd-acorr-fwd-L65-M64-fmt2": (1.10e-16, 5.01e-08),
    "acorr_fwd-acorr-fwd-L65-M64-fmt3": (7.46e-17, 6.36e-08),
    "acorr_fwd-acorr-fwd-L257-M0-fmt0": (2.12e-16, 5.42e-08),
    "acorr_fwd-acorr-fwd-L257-M0-fmt1": (0.00e+00, 0.00e+00),
    "acorr_fwd-acorr-fwd-L257-M0-fmt2": (2.10e-16, 8.77e-08),
    "acorr_fwd-acorr-fwd-L257-M0-fmt3": (2.12e-16, 2.02e-07),
    "acorr_fwd-acorr-fwd-L257-M7-fmt0": (1.90e-16, 4.66e-08),
    "acorr_fwd-acorr-fwd-L257-M7-fmt1": (3.82e-17, 8.04e-09),
    "acorr_fwd-acorr-fwd-L257-M7-fmt2": (1.86e-16, 2.17e-08),
    "acorr_fwd-acorr-fwd-L257-M7-fmt3": (9.49e-17, 5.18e-08),
    "acorr_fwd-acorr-fwd-L257-M256-fmt0": (1.16e-16, 4.02e-08),
    "acorr_fwd-acorr-fwd-L257-M256-fmt1": (6.25e-17, 2.13e-08),
    "acorr_fwd-acorr-fwd-L257-M256-fmt2": (2.07e-16, 3.81e-08),
    "acorr_fwd-acorr-fwd-L257-M256-fmt3": (3.78e-17, 2.73e-08),
    "acorr_bwd-acorr-bwd-L1-M0-fmt0": (0.00e+00, 1.51e-08),
    "acorr_bwd-acorr-bwd-L1-M0-fmt2": (0.00e+00, 1.16e-08),
    "acorr_bwd-acorr-bwd-L1-M0-fmt3": (0.00e+00, 1.25e-08),
    "acorr_bwd-acorr-bwd-L63-M0-fmt0": (0.00e+00, 4.39e-08),
    "acorr_bwd-acorr-bwd-L63-M0-fmt2": (0.00e+00, 5.49e-08),
    "acorr_bwd-acorr-bwd-L63-M0-fmt3": (0.00e+00, 4.85e-08),
    "acorr_bwd-acorr-bwd-L63-M7-fmt0": (2.92e-16, 1.25e-07),
    "acorr_bwd-acorr-bwd-L63-M7-fmt1": (1.70e-16, 1.14e-07),
    "acorr_bwd-acorr-bwd-L63-M7-fmt2": (2.10e-16, 1.01e-07),
    "acorr_bwd-acorr-bwd-L63-M7-fmt3": (2.24e-16, 1.82e-07),
    "acorr_bwd-acorr-bwd-L63-M62-fmt0": (6.25e-16, 2.34e-07),
    "acorr_bwd-acorr-bwd-L63-M62-fmt1": (6.95e-16, 2.18e-07),
    "acorr_bwd-acorr-bwd-L63-M62-fmt2": (4.82e-16, 1.80e-07),
    "acorr_bwd-acorr-bwd-L63-M62-fmt3": (1.62e-16, 2.50e-07),
    "acorr_bwd-acorr-bwd-L64-M0-fmt0": (0.00e+00, 4.02e-08),
    "acorr_bwd-acorr-bwd-L64-M0-fmt2": (0.00e+00, 4.15e-08),
    "acorr_bwd-acorr-bwd-L64-M0-fmt3": (0.00e+00, 5.73e-08),
    "acorr_bwd-acorr-bwd-L64-M7-fmt0": (2.66e-16, 1.89e-07),
    "acorr_bwd-acorr-bwd-L64-M7-fmt1": (2.83e-16, 1.87e-07),
    "acorr_bwd-acorr-bwd-L64-M7-fmt2": (3.84e-16, 1.25e-07),
    "acorr_bwd-acorr-bwd-L64-M7-fmt3": (3.24e-16, 2.26e-07),
    "acorr_bwd-acorr-bwd-L64-M63-fmt0": (3.52e-16, 2.34e-07),
    "acorr_bwd-acorr-bwd-L64-M63-fmt1": (6.82e-16, 2.51e-07),
    "acorr_bwd-acorr-bwd-L64-M63-fmt2": (3.33e-16, 1.88e-07),
    "acorr_bwd-acorr-bwd-L64-M63-fmt3": (3.47e-16, 9.79e-08),
    "acorr_bwd-acorr-bwd-L65-M0-fmt0": (0.00e+00, 4.23e-08),
    "acorr_bwd-acorr-bwd-L65-M0-fmt2": (0.00e+00, 4.69e-08),
    "acorr_bwd-acorr-bwd-L65-M0-fmt3": (0.00e+00, 5.81e-08),
    "acorr_bwd-acorr-bwd-L65-M7-fmt0": (2.89e-16, 1.37e-07),
    "acorr_bwd-acorr-bwd-L65-M7-fmt1": (2.78e-16, 1.64e-07),
    "acorr_bwd-acorr-bwd-L65-M7-fmt2": (3.24e-16, 1.48e-07),
    "acorr_bwd-acorr-bwd-L65-M7-fmt3": (2.57e-16, 1.74e-07),
    "acorr_bwd-acorr-bwd-L65-M64-fmt0": (4.71e-16, 4.07e-07),
    "acorr_bwd-acorr-bwd-L65-M64-fmt1": (6.45e-16, 2.39e-07),
    "acorr_bwd-acorr-bwd-L65-M64-fmt2": (5.20e-16, 2.24e-07),
    "acorr_bwd-acorr-bwd-L65-M64-fmt3": (4.85e-16, 9.23e-08),
    "acorr_bwd-acorr-bwd-L257-M0-fmt0": (0.00e+00, 2.93e-08),
    "acorr_bwd-acorr-bwd-L257-M0-fmt2": (0.00e+00, 5.11e-08),
    "acorr_bwd-acorr-bwd-L257-M0-fmt3": (0.00e+00, 4.06e-08),
    "acorr_bwd-acorr-bwd-L257-M7-fmt0": (2.93e-16, 1.51e-07),
    "acorr_bwd-acorr-bwd-L257-M7-fmt1": (2.17e-16, 1.44e-07),
    "acorr_bwd-acorr-bwd-L257-M7-fmt2": (3.22e-16, 1.51e-07),
    "acorr_bwd-acorr-bwd-L257-M7-fmt3": (3.13e-16, 1.76e-07),
    "acorr_bwd-acorr-bwd-L257-M256-fmt0": (1.51e-15, 3.70e-07),
    "acorr_bwd-acorr-bwd-L257-M256-fmt1": (1.42e-15, 3.35e-07),
    "acorr_bwd-acorr-bwd-L257-M256-fmt2": (1.01e-15, 3.92e-07),
    "acorr_bwd-acorr-bwd-L257-M256-fmt3": (6.37e-16, 5.10e-07),
    "acorr_bwd-lpc-bwd-L348-M86-eps1e-05": (1.83e-15, 5.14e-07),
    "acorr_bwd-lpc-bwd-L404-M100-eps1e-05": (1.99e-15, 3.72e-07),
    "frame_window_lpc_fwd-fwlpc-fwd-T250-L50-P20-M24-eps1e-05-onlyf64": (2.43e-15, 0.00e+00),
    "frame_window_lpc_fwd-fwlpc-fwd-T250-L50-P20-M23-eps1e-05-onlyf32": (0.00e+00, 1.64e-06),
    "frame_window_lpc_fwd-fwlpc-fwd-T250-L64-P20-M63-eps1e-05-centerFalse": (3.87e-15, 2.07e-06),
    "frame_window_lpc24_fwd-fwlpc-fwd-T250-L50-P20-M24-eps1e-05-exactTrue-onlyf32": (0.00e+00, 6.71e-07),
    "row_dft_generic-fftr-fwd-len_in6-nfft12-fmt0": (2.23e-16, 5.54e-08),
    "row_dft_generic-fftr-fwd-len_in12-nfft12-fmt0": (1.35e-16, 7.09e-08),
    "row_dft_generic-fftr-fwd-len_in17-nfft12-fmt0": (2.04e-16, 8.73e-08),
    "row_dft_generic-fftr-fwd-len_in8-nfft16-fmt0": (1.15e-16, 4.89e-08),
    "row_dft_generic-fftr-fwd-len_in16-nfft16-fmt0": (2.94e-16, 7.14e-08),
    "row_dft_generic-fftr-fwd-len_in21-nfft16-fmt0": (1.98e-16, 9.15e-08),
    "row_dft_generic-fftr-fwd-len_in15-nfft30-fmt0": (2.36e-16, 1.18e-07),
    "row_dft_generic-fftr-fwd-len_in30-nfft30-fmt0": (3.13e-16, 1.24e-07),
    "row_dft_generic-fftr-fwd-len_in35-nfft30-fmt0": (4.72e-16, 1.39e-07),
    "row_dft_generic-fftr-fwd-len_in35-nfft30-fmt1": (4.72e-16, 1.19e-07),
    "row_dft_generic-fftr-fwd-len_in35-nfft30-fmt2": (1.77e-16, 1.39e-07),
    "row_dft_generic-fftr-fwd-len_in35-nfft30-fmt3": (4.64e-16, 1.22e-07),
    "row_dft_generic-fftr-fwd-len_in35-nfft30-fmt4": (9.69e-16, 1.42e-07),
    "row_dft_generic-spec-fwd-lb35-la0-nfft30-eps1e-06-floor-20.0-fmt0": (2.56e-16, 1.55e-07),
    "row_dft_generic-stft-fwd-T100-L20-P7-nfft30": (4.47e-16, 4.22e-07),
    "row_fft_generic-fftr-fwd-len_in16-nfft32-fmt0": (2.17e-16, 9.92e-08),
    "row_fft_generic-fftr-fwd-len_in32-nfft32-fmt0": (2.33e-16, 6.34e-08),
    "row_fft_generic-fftr-fwd-len_in37-nfft32-fmt0": (2.65e-16, 2.10e-07),
    "row_fft_generic-fftr-fwd-len_in32-nfft64-fmt0": (4.21e-16, 1.39e-07),
    "row_fft_generic-fftr-fwd-len_in64-nfft64-fmt0": (5.20e-16, 2.31e-07),
    "row_fft_generic-fftr-fwd-len_in69-nfft64-fmt0": (5.83e-16, 1.91e-07),
    "row_fft_generic-fftr-fwd-len_in37-nfft32-fmt1": (2.65e-16, 2.10e-07),
    "row_fft_generic-fftr-fwd-len_in37-nfft32-fmt2": (3.00e-16, 1.15e-07),
    "row_fft_generic-fftr-fwd-len_in37-nfft32-fmt3": (2.65e-16, 2.10e-07),
    "row_fft_generic-fftr-fwd-len_in37-nfft32-fmt4": (4.76e-16, 3.72e-07),
    "row_fft_generic-spec-fwd-lb37-la0-nfft32-eps1e-06-floor-20.0-fmt0": (5.90e-16, 1.57e-07),
    "row_fft_generic-stft-fwd-T100-L20-P7-nfft32": (4.47e-16, 4.22e-07),
    "row_dft_bwd_generic-fftr-bwd-len_in6-nfft12-fmt0": (1.34e-16, 8.10e-08),
    "row_dft_bwd_generic-fftr-bwd-len_in12-nfft12-fmt0": (2.00e-16, 6.03e-08),
    "row_dft_bwd_generic-fftr-bwd-len_in17-nfft12-fmt0": (2.00e-16, 6.03e-08),
    "row_dft_bwd_generic-fftr-bwd-len_in8-nfft16-fmt0": (1.23e-16, 1.14e-07),
    "row_dft_bwd_generic-fftr-bwd-len_in16-nfft16-fmt0": (2.13e-16, 9.85e-08),
    "row_dft_bwd_generic-fftr-bwd-len_in21-nfft16-fmt0": (2.13e-16, 9.85e-08),
    "row_dft_bwd_generic-fftr-bwd-len_in15-nfft30-fmt0": (1.77e-16, 7.54e-08),
    "row_dft_bwd_generic-fftr-bwd-len_in30-nfft30-fmt0": (2.63e-16, 8.50e-08),
    "row_dft_bwd_generic-fftr-bwd-len_in35-nfft30-fmt0": (2.63e-16, 8.50e-08),
    "row_dft_bwd_generic-fftr-bwd-len_in35-nfft30-fmt1": (1.40e-16, 6.93e-08),
    "row_dft_bwd_generic-fftr-bwd-len_in35-nfft30-fmt2": (3.70e-16, 1.25e-07),
    "row_dft_bwd_generic-fftr-bwd-len_in35-nfft30-fmt3": (3.74e-16, 1.74e-07),
    "row_dft_bwd_generic-fftr-bwd-len_in35-nfft30-fmt4": (3.85e-16, 1.43e-07),
    "row_dft_bwd_generic-spec-bwd-lb35-la0-nfft30-eps1e-06-floor-20.0-fmt0": (5.44e-16, 4.54e-07),
    "row_fft_bwd_generic-fftr-bwd-len_in16-nfft32-fmt0": (1.63e-16, 1.74e-07),
    "row_fft_bwd_generic-fftr-bwd-len_in32-nfft32-fmt0": (2.81e-16, 1.50e-07),
    "row_fft_bwd_generic-fftr-bwd-len_in37-nfft32-fmt0": (2.81e-16, 1.50e-07),
    "row_fft_bwd_generic-fftr-bwd-len_in32-nfft64-fmt0": (3.34e-16, 1.58e-07),
    "row_fft_bwd_generic-fftr-bwd-len_in64-nfft64-fmt0": (3.34e-16, 1.93e-07),
    "row_fft_bwd_generic-fftr-bwd-len_in69-nfft64-fmt0": (3.34e-16, 1.93e-07),
    "row_fft_bwd_generic-fftr-bwd-len_in37-nfft32-fmt1": (2.85e-16, 9.35e-08),
    "row_fft_bwd_generic-fftr-bwd-len_in37-nfft32-fmt2": (2.36e-16, 1.05e-07),
    "row_fft_bwd_generic-fftr-bwd-len_in37-nfft32-fmt3": (2.56e-16, 1.57e-07),
    "row_fft_bwd_generic-fftr-bwd-len_in37-nfft32-fmt4": (3.11e-16, 1.77e-07),
    "row_fft_bwd_generic-spec-bwd-lb37-la0-nfft32-eps1e-06-floor-20.0-fmt0": (4.10e-16, 2.12e-07),
    "spec_ratio-spec-fwd-lb5-la3-nfft16-eps0.001-floorNone-fmt3": (3.90e-16, 1.14e-07),
    "spec_ratio-spec-fwd-lb3-la6-nfft30-eps0.0-floorNone-fmt0": (2.84e-16, 1.76e-07),
    "spec_ratio-spec-fwd-lb0-la4-nfft16-eps0.0-floor-30.0-fmt1": (2.88e-16, 1.80e-07),
    "spec_ratio_bwd-spec-bwd-lb5-la3-nfft16-eps0.001-floorNone-fmt3": (3.94e-16, 1.98e-07),
    "spec_ratio_bwd-spec-bwd-lb3-la6-nfft30-eps0.0-floorNone-fmt0": (3.99e-16, 1.15e-07),
    "spec_ratio_bwd-spec-bwd-lb0-la4-nfft16-eps0.0-floor-30.0-fmt1": (1.88e-16, 8.78e-08),
    "window_grad_colsum-stft-bwd-T100-L20-P7-nfft30": (3.33e-16, 1.13e-07),
    "window_grad_colsum-stft-bwd-T100-L20-P7-nfft32": (2.70e-16, 1.84e-07),
    "irfft_scale-irfft_scale-fwd-nfft2": (0.00e+00, 0.00e+00),
    "irfft_scale-irfft_scale-fwd-nfft30": (0.00e+00, 3.62e-08),
    "th_solve_bwd-thsolve-bwd-n1-onlyf64": (0.00e+00, 0.00e+00),
    "th_solve_bwd-thsolve-bwd-n24-onlyf64": (6.59e-16, 0.00e+00),
    "th_solve_bwd-thsolve-bwd-n25-onlyf64": (7.94e-16, 0.00e+00),
    "th_solve_bwd-thsolve-bwd-n64-onlyf64": (1.57e-15, 0.00e+00),
    "th_solve_bwd-thsolve-bwd-n1-onlyf32": (0.00e+00, 4.10e-08),
    "th_solve_bwd-thsolve-bwd-n56-onlyf32": (0.00e+00, 3.78e-07),
    "th_solve_bwd-thsolve-bwd-n64-onlyf32": (0.00e+00, 3.81e-07),
    "th_solve_quad_bwd-thsolve-bwd-n24-onlyf32": (0.00e+00, 3.66e-07),
    "th_solve_quadn_bwd-thsolve-bwd-n2-onlyf32": (0.00e+00, 2.35e-07),
    "th_solve_quadn_bwd-thsolve-bwd-n23-onlyf32": (0.00e+00, 3.50e-07),
    "th_solve_quadn_bwd-thsolve-bwd-n25-onlyf32": (0.00e+00, 3.98e-07),
    "th_solve_quadn_bwd-thsolve-bwd-n55-onlyf32": (0.00e+00, 3.78e-07),
    "freqt_lds_fwd-freqt-fwd-L148-L225": (2.97e-16, 1.79e-07),
    "freqt_lds_fwd-freqt-fwd-L149-L225-onlyf64": (7.00e-16, 0.00e+00),
    "freqt_fwd-freqt-fwd-L1400-L240-onlyf32": (0.00e+00, 5.27e-07),
    "freqt_fwd-freqt-fwd-L1100-L270-onlyf64": (7.53e-16, 0.00e+00),
    "freqt_lds_bwd-freqt-bwd-L148-L225": (3.45e-16, 1.11e-07),
    "freqt_lds_bwd-freqt-bwd-L149-L225": (3.55e-16, 1.02e-07),
    "freqt_bwd-freqt-bwd-L1400-L240-onlyf32": (0.00e+00, 1.79e-07),
    "freqt_bwd-freqt-bwd-L1100-L270-onlyf64": (6.63e-16, 0.00e+00),
    "rows_log-rows_log-fwd-n300-onlyf32": (0.00e+00, 5.16e-08),
    "rows_log-rows_log-bwd-n300-onlyf32": (0.00e+00, 7.88e-08),
    "rows_expsub-rows_expsub-fwd-n300-onlyf32": (0.00e+00, 2.02e-08),
    "rows_expsub-rows_expsub-bwd-n300-onlyf32": (0.00e+00, 7.73e-08),
    "fbank_bwd-fbank-bwd-nfft64-C12-use_powerFalse-gamma0.0": (1.61e-16, 1.08e-07),
    "fbank_bwd-fbank-bwd-nfft64-C12-use_powerTrue-gamma-0.5": (8.63e-17, 8.99e-08),
    "fbank_bins_bwd-fbank_bins-bwd-nfft64-C12-gamma0.0-onlyf32": (0.00e+00, 7.25e-08),
    "fbank_bins_bwd-fbank_bins-bwd-nfft64-C12-gamma-0.5-onlyf32": (0.00e+00, 7.85e-08),
    "mgcep_step-mgcep_step-fwd-nfft512-M24-gamma-0.5-onlyf32": (0.00e+00, 4.61e-07),
    "mgcep_step-mgcep_step-fwd-nfft512-M17-gamma-0.5-onlyf32": (0.00e+00, 5.53e-07),
    "mgcep_step_bwd-mgcep_step-bwd-nfft512-M17-gamma-0.5-onlyf32": (0.00e+00, 2.84e-07),
    "mgcep_spectra-mgcep_spectra-fwd-nfft64-M8-gamma-0.5": (2.42e-16, 1.23e-07),
    "mgcep_spectra-mgcep_spectra-fwd-nfft64-M32-gamma-0.5": (4.10e-16, 1.88e-07),
    "mgcep_gain-mgcep_gain-fwd-M1-gamma-0.5": (0.00e+00, 5.36e-08),
    "mgcep_gain-mgcep_gain-fwd-M24-gamma-0.5": (0.00e+00, 3.13e-08),
    "mcep_newton_update_bwd-newton_update-bwd-n7-onlyf32": (0.00e+00, 2.46e-07),
    "mcep_newton_update_bwd-newton_update-bwd-n35-onlyf32": (0.00e+00, 3.40e-07),
    "poledf_generic_bwd-poledf-bwd-M0-P16-N3-igFalse": (0.00e+00, 7.30e-08),
    "poledf_generic_bwd-poledf-bwd-M64-P16-N3-igTrue": (0.00e+00, 1.32e-07),
    "interpolate_fwd-interpolate-fwd-T7-P3-s2": (0.00e+00, 0.00e+00),
    "interpolate_bwd-interpolate-bwd-T7-P3-s2": (0.00e+00, 3.75e-08),
    "delta_bwd-delta-bwd-T9-D3-seedw23": (0.00e+00, 1.37e-07),
    "mlpg_adjoint_any-mlpg-bwd-T30-D3-seedw5": (4.85e-16, 1.93e-07),
    "mdct_analysis_fast-mdct-fwd-L16-T50-onlyf32": (0.00e+00, 8.18e-08),
    "mdct_analysis_generic-mdct-fwd-L16-T50-onlyf64": (2.26e-16, 0.00e+00),
    "mdct_analysis_generic-mdct-fwd-L12-T50": (2.72e-16, 1.07e-07),
    "mdct_synthesis_fast-imdct-fwd-L16-N7-onlyf32": (0.00e+00, 1.11e-07),
    "mdct_synthesis_generic-imdct-fwd-L16-N7-onlyf64": (2.26e-16, 0.00e+00),
    "mdct_synthesis_generic-imdct-fwd-L12-N7": (1.69e-16, 6.78e-08),
    # ---- CEILINGS, both sides
    "acorr_fwd-acorr-fwd-L15360-M2-fmt0-F1-onlyf32": (0.00e+00, 1.63e-08),
    "acorr_fwd-acorr-fwd-L7680-M2-fmt0-F1-onlyf64": (1.83e-18, 0.00e+00),
    "acorr_bwd-acorr-bwd-L15354-M2-fmt0-F1-onlyf32": (0.00e+00, 8.42e-08),
    "acorr_bwd-acorr-bwd-L7677-M2-fmt0-F1-onlyf64": (1.25e-16, 0.00e+00),
    "levdur_fwd_lds-levdur-fwd-M2559-eps1e-05-F1": (2.66e-19, 9.21e-09),
    "levdur_bwd_toeplitz-levdur-bwd-M1097-eps1e-05-F1": (2.77e-15, 9.24e-07),
    "frame_window_lpc_fwd-fwlpc-fwd-L3840-T4000-P2000-M8-eps1e-05-B1-onlyf32": (0.00e+00, 7.51e-08),
    "frame_window_lpc_fwd-fwlpc-fwd-L1920-T4000-P2000-M8-eps1e-05-B1-onlyf64": (1.38e-17, 0.00e+00),
    "levdur_fwd-fuse_fwlpc-fwd-L3841-T4000-P2000-M8-eps1e-05-B1-onlyf32": (0.00e+00, 1.56e-08),
    "levdur_fwd-fuse_fwlpc-fwd-L1921-T4000-P2000-M8-eps1e-05-B1-onlyf64": (4.15e-17, 0.00e+00),
    "row_dft_generic-fftr-fwd-len_in15360-nfft30-fmt0-F1-onlyf32": (0.00e+00, 8.22e-08),
    "row_dft_generic-fftr-fwd-len_in7680-nfft30-fmt0-F1-onlyf64": (3.35e-16, 0.00e+00),
    "row_dft_bwd_generic-fftr-bwd-len_in15312-nfft30-fmt0-F1-onlyf32": (0.00e+00, 9.04e-08),
    "row_dft_bwd_generic-fftr-bwd-len_in7632-nfft30-fmt0-F1-onlyf64": (0.00e+00, 0.00e+00),
    "row_fft_generic-fftr-fwd-len_in30208-nfft4096-fmt0-F1-onlyf32": (0.00e+00, 3.32e-07),
    "row_fft_generic-fftr-fwd-len_in11008-nfft4096-fmt0-F1-onlyf64": (1.19e-15, 0.00e+00),
    "row_fft_generic-fftr-fwd-len_in2816-nfft8192-fmt0-F1-onlyf64": (1.08e-15, 0.00e+00),
    "row_fft_generic-fftr-fwd-len_in5632-nfft16384-fmt0-F1-onlyf32": (0.00e+00, 4.64e-07),
    "row_dft_generic-fftr-fwd-len_in2817-nfft8192-fmt0-F1-onlyf64": (1.11e-15, 0.00e+00),
    "row_dft_generic-fftr-fwd-len_in5633-nfft16384-fmt0-F1-onlyf32": (0.00e+00, 4.44e-07),
    "row_fft_bwd_generic-fftr-bwd-len_in24061-nfft4096-fmt0-F1-onlyf32": (0.00e+00, 1.55e-07),
    "row_fft_bwd_generic-fftr-bwd-len_in4861-nfft4096-fmt0-F1-onlyf64": (3.57e-16, 0.00e+00),
    "spec_ratio_bwd-spec-bwd-nfft6138-lb5-la3-eps0.001-floorNone-fmt3-F2-onlyf32": (0.00e+00, 2.36e-07),
    "spec_ratio_bwd-spec-bwd-nfft3066-lb5-la3-eps0.001-floorNone-fmt3-F2-onlyf64": (8.15e-16, 0.00e+00),
    "fbank_fwd-fbank-fwd-nfft4778-C80-use_powerFalse-gamma0.0-F13-onlyf32": (0.00e+00, 2.40e-07),
    "fbank_fwd-fbank-fwd-nfft2388-C80-use_powerFalse-gamma0.0-F13-onlyf64": (4.13e-16, 0.00e+00),
    "fbank_bwd-fbank-bwd-nfft4104-C80-use_powerFalse-gamma0.0-F13-onlyf32": (0.00e+00, 1.73e-07),
    "fbank_bwd-fbank-bwd-nfft2096-C80-use_powerFalse-gamma0.0-F13-onlyf64": (2.76e-16, 0.00e+00),
    "fbank_fwd-fbank-fwd-nfft794-C80-use_powerFalse-gamma0.0-F13-onlyf32": (0.00e+00, 1.99e-07),
    "fbank_fwd-fbank-fwd-nfft396-C80-use_powerFalse-gamma0.0-F13-onlyf64": (3.71e-16, 0.00e+00),
    "fbank_bwd-fbank-bwd-nfft752-C80-use_powerFalse-gamma0.0-F13-onlyf32": (0.00e+00, 1.18e-07),
    "fbank_bwd-fbank-bwd-nfft364-C80-use_powerFalse-gamma0.0-F13-onlyf64": (1.71e-16, 0.00e+00),
    "fbank_fwd-fbank-fwd-nfft796-C80-use_powerFalse-gamma0.0-F13-onlyf32": (0.00e+00, 2.64e-07),
    "fbank_fwd-fbank-fwd-nfft398-C80-use_powerFalse-gamma0.0-F13-onlyf64": (8.00e-16, 0.00e+00),
    "fbank_bwd-fbank-bwd-nfft754-C80-use_powerFalse-gamma0.0-F13-onlyf32": (0.00e+00, 1.39e-07),
    "fbank_bwd-fbank-bwd-nfft366-C80-use_powerFalse-gamma0.0-F13-onlyf64": (1.67e-16, 0.00e+00),
    "fbank_fwd-fbank-fwd-nfft1024-C80-use_powerFalse-gamma0.0-F64-onlyf32": (0.00e+00, 3.15e-07),
    "fbank_bwd-fbank-bwd-nfft1024-C80-use_powerFalse-gamma0.0-F64-onlyf32": (0.00e+00, 1.37e-07),
    "fbank_fwd-fbank-fwd-nfft640-C12-use_powerFalse-gamma0.0-F5-onlyf32": (0.00e+00, 2.91e-07),
    "plp_bwd-plp_tail-bwd-n_fft3538-C20-M12-F5-onlyf32": (0.00e+00, 2.56e-07),
    "plp_bwd-plp_tail-bwd-n_fft1704-C20-M12-F5-onlyf64": (1.38e-15, 0.00e+00),
    "plp_bwd-plp_tail-bwd-n_fft3540-C20-M12-F5-onlyf32": (0.00e+00, 2.55e-07),
    "plp_bwd-plp_tail-bwd-n_fft1706-C20-M12-F5-onlyf64": (1.96e-15, 0.00e+00),
    "plp_bwd-plp_tail-bwd-n_fft7634-C20-M12-F5-onlyf32": (0.00e+00, 3.27e-07),
    "plp_bwd-plp_tail-bwd-n_fft3752-C20-M12-F5-onlyf64": (1.38e-15, 0.00e+00),
    "plp_bwd-plp_tail-bwd-n_fft7636-C20-M12-F5-onlyf32": (0.00e+00, 2.55e-07),
    "plp_bwd-plp_tail-bwd-n_fft3754-C20-M12-F5-onlyf64": (6.92e-16, 0.00e+00),
    "plp_bwd-plp_tail-bwd-n_fft40402-C20-M12-F5-onlyf32": (0.00e+00, 3.99e-07),
    "plp_bwd-plp_tail-bwd-n_fft20136-C20-M12-F5-onlyf64": (1.56e-15, 0.00e+00),
    "mlsacheck_generic_fwd-mlsacheck-fwd-M9214-modefast-n_fft256-F3": (1.28e-16, 2.13e-07),
    "mlsacheck_generic_bwd-mlsacheck-bwd-M6142-modefast-n_fft256-F3": (0.00e+00, 9.07e-08),
    "mgcep_spectra-mgcep_spectra-fwd-nfft256-M64-gamma-0.5-F3": (4.23e-16, 1.06e-07),
    "mcep_generic_fwd-mcep_generic-fwd-nfft27208-M8-alpha0.42-n_iter2-F2-onlyf32": (0.00e+00, 1.74e-06),
    "mcep_generic_fwd-mcep_generic-fwd-nfft13556-M8-alpha0.42-n_iter2-F2-onlyf64": (5.12e-15, 0.00e+00),
    "mcep_generic_bwd-mcep_generic-bwd-nfft27208-M8-alpha0.42-n_iter2-F2-onlyf32": (0.00e+00, 5.85e-07),
    "mcep_generic_bwd-mcep_generic-bwd-nfft13556-M8-alpha0.42-n_iter2-F2-onlyf64": (1.70e-15, 0.00e+00),
    "mdct_analysis_fast-mdct-fwd-L4096-T5000-B1-onlyf32": (0.00e+00, 3.34e-07),
    "mdct_synthesis_fast-imdct-fwd-L4096-N3-B1-onlyf32": (0.00e+00, 2.74e-07),
    "mdct_analysis_generic-mdct-fwd-L8192-T9000-B1-onlyf32": (0.00e+00, 3.99e-07),
    "mdct_synthesis_generic-imdct-fwd-L8192-N3-B1-onlyf32": (0.00e+00, 3.02e-07),
    "mlsacheck_generic_fwd-mlsacheck-fwd-M24-modescale-n_fft18380-F3": (2.48e-16, 7.89e-08),
    "mlsacheck_generic_bwd-mlsacheck-bwd-M24-modescale-n_fft18354-F3": (4.79e-16, 2.33e-07),
    "mlsacheck_generic_fwd-mlsacheck-fwd-M24-modeclip-n_fft18380-F3": (3.33e-16, 7.81e-08),
    "mlsacheck_generic_bwd-mlsacheck-bwd-M24-modeclip-n_fft18354-F3": (4.79e-16, 2.33e-07),
}
