"""The capped grids' table, names and numbers only.  Every `__global__` kernel of diffsptk_amd/csrc/*.hip and *.h whose body
mentions `gridDim.` walks its rows, tiles, utterances or elements in a grid-stride loop, and its launcher clamps the grid to a
constant: a batch above that constant sends a workgroup (or a wave) through the loop body a second time.  Every such kernel is in
exactly one of

  CAPPED            kernel -> the source file, the launcher's cap as it is spelled there, what one grid slot covers in one trip
                    (`trip` units of `unit`), and the cases that pass the cap (tests/test_gpu_grid_strides.py runs them)
  PINNED_ELSEWHERE  kernel -> an existing test that passes the cap (checked by reading the launcher), with the rows it runs and the
                    trips that makes; grids that depend on the device are counted at the MI355X's 256 CUs
  OUT_OF_REACH      kernel -> why no test of a few seconds passes the cap, with the bytes of the smallest case (at most 8)

tests/test_grid_strides_cpu.py checks, without a GPU, that no kernel is missing, stale or in two tables, that every cap text sizes a
grid in the file the entry names, and that every case's batch exceeds its cap.

A case: the family (a key of FAMILIES in tests/test_gpu_grid_strides.py: the public call, the family's own generator of benign rows,
its float64 reference and its bound), "fwd" or "bwd", the dtypes, the smallest row shape that still reaches the kernel, `per_row`
(units of the entry that one row of the batch brings: 1 unless a row is an utterance of several elements), the route
`_lib.last_kernel()` must report, and whether include/diffsptk_amd.h promises that a row's bits depend on the row alone (`promised`;
where it does not, the big call is compared with two calls on slices under the cap instead of with the 251-row call).  The batches
follow from the cap: B = rows(cap) + 3, and 2 rows(cap) + 1 (a third trip) where that stays below 64 MiB per tensor.  SECONDS, at
the end, holds the time of every case on an MI355X (its preparation, every batch, the references and the flag runs included) as
measured when the table was written: a case that no longer finishes in a few seconds belongs in OUT_OF_REACH with its figure."""

PRIME = 251   # distinct rows per case: prime, and no rows(cap) is a multiple of it, so rows f and f + rows(cap) always differ


def rows_of_cap(entry, c):
    """batch rows that fill the capped grid once"""
    # ("256L * 16" is C++ for 256 * 16; a cap spelled with a variable carries its largest value beside the text)
    units = entry.get("cap_value", None) or eval(entry["cap"].replace("L", ""), {})
    units *= entry["trip"]
    return -(-units // c.get("per_row", 1))


def batches(entry, c):
    n = rows_of_cap(entry, c)
    return (n + 3, 2 * n + 1) if c.get("third_trip") else (n + 3,)


def case(family, when, dtypes, route, promised=True, **kw):
    extra = {k: kw.pop(k) for k in ("per_row", "third_trip", "fwd_route", "flag") if k in kw}
    return dict(family=family, when=when, dtypes=dtypes, route=route, promised=promised, shape=kw, **extra)


def case_id(kernel, c):
    return "-".join([kernel, c["family"], c["when"]] + [f"{k}{v}" for k, v in c["shape"].items() if k not in ("rows", "batch", "spec")]
                    + ["".join(f"{k}{v}" for k, v in c["shape"].get("spec", (0, 0, ()))[2])] * ("spec" in c["shape"]))


BOTH, F32, F64 = ("f32", "f64"), ("f32",), ("f64",)


def like(case_id_of_kernel_routes, when=None, **kw):
    """a case of tests/kernel_routes.py by its id, at 251 and at B rows: its call, inputs, float64 restatement and bound; `batch` is
    the argument that carries the batch, `rows` the inputs with one row per batch entry.  (`when` only says, for the reader, that a
    backward case of that table is run forward here: its bound is a family's own and covers the outputs.)"""
    return dict(like=case_id_of_kernel_routes, **kw)


def _mlsa(kind, dtypes, shapes, cap_small):
    """forward (with the unstable flag) and backward cases of one mlsacheck kernel"""
    return [case("mlsacheck", when, dtypes, f"mlsacheck_{kind}_{when}", third_trip=cap_small, **dict(s, **({"flag": "unstable"} if when == "fwd" else {})))
            for s in shapes for when in ("fwd", "bwd")]


def _parcor():
    """the six ops of parcor_row_kernel at M = DSA_PARCOR_MAX_ORDER + 1 = 33 (about 140 MiB per float32 tensor)"""
    out = []
    for op in ("lpc2par", "par2lpc", "lpccheck"):
        for when in ("fwd", "bwd"):
            out.append(case("parcor", when, BOTH, f"parcor_row_{op}_{when}", op=op, M=33,
                            **({"flag": "unstable"} if (op, when) == ("lpccheck", "fwd") else {})))
    return out


CAPPED = {
    # ---- csrc/mlsacheck.hip: one frame per one-wave workgroup.  tuned: float32, M <= 63, fast mode or n_fft 256; generic: the rest
    "mlsacheck_tuned_kernel": dict(file="mlsacheck.hip", cap="1 << 14", trip=1, unit="frame",
                                   cases=_mlsa("tuned", F32, [dict(M=3, mode="fast", n_fft=256), dict(M=3, mode="clip", n_fft=256)], True)),
    "mlsacheck_generic_kernel": dict(file="mlsacheck.hip", cap="1 << 16", trip=1, unit="frame",
                                     cases=_mlsa("generic", F64, [dict(M=3, mode="fast", n_fft=256)], True)
                                     + _mlsa("generic", BOTH, [dict(M=3, mode="scale", n_fft=8), dict(M=3, mode="clip", n_fft=8)], True)),
    # ---- csrc/excite.hip: one utterance per workgroup; the run's sum is carried from chunk to chunk and must restart per utterance
    "excite_kernel": dict(file="excite.hip", cap="1 << 16", trip=1, unit="utterance",
                          cases=[case("excite", "fwd", BOTH, "excite_{dt}", third_trip=True, N=5, P=2)]),
    # ---- csrc/lsp.hip: one frame per one-wave workgroup, the row and the two Chebyshev series in LDS
    "lsp_lpc2lsp_fwd_kernel": dict(file="lsp.hip", cap="1 << 20", trip=1, unit="frame",
                                   cases=[case("lpc2lsp", "fwd", BOTH, "lsp_lpc2lsp_fwd", third_trip=True, M=2, flag="failed")]),
    "lsp_lpc2lsp_bwd_kernel": dict(file="lsp.hip", cap="1 << 20", trip=1, unit="frame",
                                   cases=[case("lpc2lsp", "bwd", BOTH, "lsp_lpc2lsp_bwd", third_trip=True, M=2)]),
    # ---- csrc/parcor.hip: M > DSA_PARCOR_MAX_ORDER = 32 leaves the lane kernels for one frame per workgroup
    "parcor_row_kernel": dict(file="parcor.hip", cap="1 << 20", trip=1, unit="frame", cases=_parcor()),
    # ---- csrc/paramgen.hip: one frame per one-wave workgroup
    "mcpf_fwd_kernel": dict(file="paramgen.hip", cap="1 << 20", trip=1, unit="frame",
                            cases=[case("mcpf", "fwd", BOTH, "mcpf_fwd", third_trip=True, M=1, alpha=0.42, beta=0.2, onset=1, ir_length=8)]),
    "mcpf_bwd_kernel": dict(file="paramgen.hip", cap="1 << 20", trip=1, unit="frame",
                            cases=[case("mcpf", "bwd", BOTH, "mcpf_bwd", third_trip=True, M=1, alpha=0.42, beta=0.2, onset=1, ir_length=8)]),
    # ---- csrc/stft.hip and its headers.  fft_length 512 with a frame length other than 400: the register-FFT kernels, persistent
    # waves that take one pass of 4 frames at a time, and the gather of the backward's spans with the utterances in grid.y.
    # Utterances of 7 samples are one frame, one pass: 65 538 of them pass all three caps.  The header promises nothing about the
    # batch for the STFT: slices.
    "stft_span_gather_kernel": dict(file="stft.hip", cap="65535", trip=1, unit="utterance",
                                    cases=[case("stft", "bwd", F32, "stft512_bwd", promised=False, L=320, P=80, nfft=512, T=7, fwd_route="stft512_fwd")]),
    "stft512_fwd_kernel": dict(file="stft.hip", cap="256L * 16", trip=1, unit="pass of 4 frames, one per wave",
                               cases=[case("stft", "fwd", F32, "stft512_fwd", promised=False, L=320, P=80, nfft=512, T=81)]),
    "stft512_bwd_kernel": dict(file="stft.hip", cap="256L * 16", trip=1, unit="pass of 4 frames, one per wave (the power format's instantiation)",
                               cases=[case("stft", "bwd", F32, "stft512_bwd", promised=False, L=320, P=80, nfft=512, T=81, fwd_route="stft512_fwd")]),
    # frame length 400: the packed kernels.  The backward's grid is min(utterances x runs, 4096 waves): 4 099 utterances of one pass
    "stft512_fwd_pk_kernel": dict(file="stft.hip", cap="256L * 16", trip=1, unit="pass of 4 frames, one per wave",
                                  cases=[case("stft", "fwd", F32, "stft512_fwd", promised=False, L=400, P=80, nfft=512, T=161)]),
    "stft512_bwd_pk_kernel": dict(file="stft.hip", cap="256L * 16", trip=1, unit="run of passes of one utterance, one per wave",
                                  cases=[case("stft", "bwd", F32, "stft512_bwd_pk", promised=False, L=400, P=80, nfft=512, T=161, fwd_route="stft512_fwd")]),
    # fft_length 2048 (48 kHz): four-wave workgroups, one pass of one frame per wave; the backward min(utterances x runs, 2048 waves)
    "stft_big_fwd_pk_kernel": dict(file="stft.hip", cap="256L * 3", trip=4, unit="pass of one frame, four per workgroup",
                                   cases=[case("stft", "fwd", F32, "stft2048_fwd", promised=False, L=1200, P=240, nfft=2048, T=240)]),
    "stft_big_bwd_pk_kernel": dict(file="stft.hip", cap="256L * 2 * 4", trip=1, unit="run of passes of one utterance, one per wave",
                                   cases=[case("stft", "bwd", F32, "stft2048_bwd", promised=False, L=1200, P=240, nfft=2048, T=240, fwd_route="stft2048_fwd")]),
    # ---- csrc/lpc24.hip: the exact-lag-sum forward deals (utterance, run of frames) items to one-wave workgroups by a ticket counter
    # that the last ticket resets: 2 051 utterances of three frames are 2 051 items on at most 2 048 waves
    "frame_window_lpc24_kernel": dict(file="lpc24.hip", cap="256L * waves_per_cu", cap_value=256 * 8, trip=1, unit="item of up to 64 frames (at most 8 waves per CU)",
                                      cases=[case("lpc_exact", "fwd", F32, "frame_window_lpc24_fwd", promised=False, T=161)]),
    # ---- csrc/griffin.hip: Unframe's division, utterances in grid.y; the phase update, 256 bins of (B, N, K) per block
    "griffin_update_kernel": dict(file="griffin.hip", cap="8192", trip=256, unit="bin",
                                  cases=[case("griffin", "fwd", F32, "stft512_bwd_pk", promised=False, N=3, n_iter=2, per_row=771),
                                         case("griffin", "fwd", F64, "div_rows", promised=False, N=3, n_iter=2, per_row=771)]),
    "div_rows_kernel": dict(file="griffin.hip", cap="1024", trip=1, unit="utterance",
                            cases=[case("unframe", "fwd", BOTH, "div_rows", promised=False, L=30, P=7, N=3)]),
    # ---- csrc/spec.hip: element-wise, 256 elements (window_vec4: 256 float4) per block and trip
    "frame_fwd_vec4_kernel": dict(file="spec.hip", cap="256 * 16", trip=1024, unit="element",
                                  cases=[case("frame", "fwd", F32, "frame_fwd_vec4", promised=False, L=400, P=80, T=161, per_row=1200)]),
    "window_fwd_kernel": dict(file="spec.hip", cap="65536", trip=256, unit="element",
                              cases=[case("window", "fwd", BOTH, "window_fwd", promised=False, L=25, per_row=25)]),
    "window_bwd_kernel": dict(file="spec.hip", cap="65536", trip=256, unit="element",
                              cases=[case("window", "bwd", BOTH, "window_bwd", promised=False, L=25, per_row=25, fwd_route="window_fwd")]),
    "window_vec4_kernel": dict(file="spec.hip", cap="16384", trip=1024, unit="element",
                               cases=[case("window", "fwd", F32, "window_vec4", promised=False, L=400, per_row=400)]),
    # ---- csrc/thsolve.hip, thsolve_quad.hip, mgcep_step.hip: the cases of tests/kernel_routes.py at 251 and at B systems.  The
    # forward kernels run in the forward of the backward cases: their solution is held bit for bit and, through the gradient that is
    # formed from it, to float64
    "th_solve_fwd_kernel": dict(file="thsolve.hip", cap="256L * 16", trip=1, unit="system",
                                cases=[case("routes", "bwd", F64, "th_solve_bwd", third_trip=True, fwd_route="th_solve_fwd",
                                            **like("th_solve_bwd-thsolve-bwd-n24-onlyf64", batch="F", rows=("p", "q", "r")))]),
    "th_solve_bwd_kernel": dict(file="thsolve.hip", cap="256L * 16", trip=1, unit="system",
                                cases=[case("routes", "bwd", F64, "th_solve_bwd", third_trip=True,
                                            **like("th_solve_bwd-thsolve-bwd-n25-onlyf64", batch="F", rows=("p", "q", "r")))]),
    "thsolve_quad24_kernel": dict(file="mgcep_step.hip", cap="256L * 4", trip=64, unit="system (four waves of 16)",
                                  cases=[case("routes", "bwd", F32, "th_solve_quad_bwd", fwd_route="th_solve_quad_fwd",
                                              **like("th_solve_quad_bwd-thsolve-bwd-n24-onlyf32", batch="F", rows=("p", "q", "r")))]),
    "thsolve_quadn_kernel": dict(file="thsolve_quad.hip", cap="256", trip=64, unit="system (four waves of 16)",
                                 cases=[case("routes", "bwd", F32, "th_solve_quadn_bwd", third_trip=True, fwd_route="th_solve_quadn_fwd",
                                             **like("th_solve_quadn_bwd-thsolve-bwd-n25-onlyf32", batch="F", rows=("p", "q", "r")))]),
    "thsolve_octn_kernel": dict(file="thsolve_quad.hip", cap="512", trip=32, unit="system (four waves of 8)",
                                cases=[case("routes", "bwd", F32, "th_solve_quadn_bwd", third_trip=True, fwd_route="th_solve_octn_fwd",
                                            **like("th_solve_quadn_bwd-thsolve-bwd-n55-onlyf32", batch="F", rows=("p", "q", "r")))]),
    # the step's adjoint on binary16 images: eight waves of 16 frames per workgroup
    "mgcep_step_bwd_h_kernel": dict(file="mgcep_step.hip", cap="256", trip=128, unit="frame (eight waves of 16)",
                                    cases=[case("mgcep_step_h", "bwd", F32, "mgcep_step_bwd_h", fwd_route="mgcep_step", M=24)]),
    # ---- csrc/mcep.hip: the LDS-resident row product, 64 rows per block
    "matmul_rows_lds_kernel": dict(file="mcep.hip", cap="1024", trip=64, unit="row",
                                   cases=[case("routes", "fwd", BOTH, "freqt_lds_fwd", **like("freqt_lds_fwd-freqt-fwd-L148-L225", batch="F", rows=("c",))),
                                          case("routes", "bwd", BOTH, "freqt_lds_bwd", **like("freqt_lds_bwd-freqt-bwd-L148-L225", batch="F", rows=("c",)))]),
    # ---- csrc/fbank.hip: persistent workgroups of up to 16 waves, 4 frames per wave and pass (K = 33 bins: all 16 waves fit);
    # the matrix-core forward 4 waves of 16 frames; the bins' backward 256 elements of (F, K) per block
    "fbank_bwd_kernel": dict(file="fbank.hip", cap="256", trip=64, unit="frame (16 waves of 4)",
                             cases=[case("routes", "bwd", BOTH, "fbank_bwd",
                                         **like("fbank_bwd-fbank-bwd-nfft64-C12-use_powerTrue-gamma-0.5", batch="F", rows=("x",)))]),
    "fbank_fwd_kernel": dict(file="fbank.hip", cap="256", trip=64, unit="frame (16 waves of 4)",
                             cases=[case("routes", "bwd", F64, "fbank_bwd", fwd_route="fbank_fwd",
                                         **like("fbank_bwd-fbank-bwd-nfft64-C12-use_powerFalse-gamma0.0", batch="F", rows=("x",)))]),
    "fbank_mfma_fwd_kernel": dict(file="fbank.hip", cap="256", trip=64, unit="frame (4 waves of 16)",
                                  cases=[case("routes", "fwd", F32, "fbank_mfma_fwd",
                                              **like("fbank_mfma_fwd-fbank-fwd-nfft638-C12-use_powerFalse-gamma0.0-F5-onlyf32", batch="F", rows=("x",))),
                                         # 33 bins: k-slot 3 lies past the row (the slot's limit was negative once, and the last row of a
                                         # workgroup's last tile -- rows 63 mod 64 -- read the LDS behind the tiles); under the bound of
                                         # the matrix-core forward's own test
                                         case("routes", "fwd", F32, "fbank_mfma_fwd", spec=("fbank", "FBM", (("nfft", 64), ("C", 12), ("use_power", True), ("gamma", -0.5))),
                                              batch="F", rows=("x",))]),
    "fbank_bins_bwd_kernel": dict(file="fbank.hip", cap="256L * 32", trip=256, unit="element of (F, K)",
                                  cases=[case("routes", "bwd", F32, "fbank_bins_bwd", per_row=33,
                                              **like("fbank_bins_bwd-fbank_bins-bwd-nfft64-C12-gamma0.0-onlyf32", batch="F", rows=("s",)))]),
    # ---- csrc/pqmf.hip (pq_blocks: 2^20 blocks of 256 elements, 1 GiB of float32 per tensor that the loop runs over).  float32
    # only: the float64 instantiation of the same loop doubles the bytes past 4 GiB
    "pqmf_fwd_generic_kernel": dict(file="pqmf.hip", cap="1L << 20", trip=256, unit="element of y",
                                    cases=[case("routes", "fwd", F32, "pqmf_fwd_generic", per_row=2700,
                                                **like("pqmf_bwd_x-pqmf-bwd-K9-M40-T300", "fwd", batch="B", rows=("x",)))]),
    # (no case of tests/kernel_routes.py reaches the generic synthesis with few bands: 129 taps do, under the family's own bound)
    "ipqmf_fwd_generic_kernel": dict(file="pqmf.hip", cap="1L << 20", trip=256, unit="element of x",
                                     cases=[case("routes", "fwd", F32, "ipqmf_fwd_generic", per_row=70,
                                                 spec=("ipqmf", "PQ", (("K", 2), ("M", 128), ("T", 70))), batch="B", rows=("y",))]),
    "ipqmf_bwd_y_kernel": dict(file="pqmf.hip", cap="1L << 20", trip=256, unit="element of gy",
                               cases=[case("routes", "bwd", F32, "ipqmf_bwd_y", per_row=280,
                                           **like("ipqmf_bwd_y-ipqmf-bwd-K4-M41-T70-U3-s1", batch="B", rows=("y",)))]),
    "interp_fwd_kernel": dict(file="pqmf.hip", cap="1L << 20", trip=256, unit="element of y",
                              cases=[case("routes", "fwd", F32, "interpolate_fwd", per_row=115,
                                          **like("interpolate_fwd-interpolate-fwd-T7-P3-s2", batch=None, rows=("x",)))]),
    # the analysis' backward with respect to x: any period other than 1 goes to the generic kernel, whatever K.  One band, period 16:
    # 1 GiB each of x and gx, 1/16 GiB each of y and its cotangent
    "pqmf_bwd_x_kernel": dict(file="pqmf.hip", cap="1L << 20", trip=256, unit="element of gx",
                              cases=[case("routes", "bwd", F32, "pqmf_bwd_x", per_row=320,
                                          spec=("pqmf", "PQ", (("K", 1), ("M", 7), ("T", 320), ("P", 16), ("s", 1))), batch="B", rows=("x",))]),
}

PINNED_ELSEWHERE = {
    # ---- csrc/dtw.hip: DTW_MAX_GRID = 1 << 16 workgroups, one pair each
    "dtw_kernel": dict(test="tests/test_gpu_dtw.py::test_more_pairs_than_the_grid_has_workgroups", rows="65 541 pairs", trips=2),
    "dtw_vjp_kernel": dict(test="tests/test_gpu_dtw.py::test_more_pairs_than_the_grid_has_workgroups", rows="65 541 pairs", trips=2),
    # ---- the flagship kernels at the benchmark's sizes: 1 024 utterances of 1 s are 204 800 frames, 51 200 passes, 12 800 tiles of 16
    "mcep_mfma_fwd_kernel_h": dict(test="tests/test_gpu_configs.py::test_config5_shard_1024_utterances",
                                   rows="204 800 frames = 12 800 tiles on 256 workgroups x 8 waves", trips=7),
    "mcep_mfma_bwd2_kernel_h": dict(test="tests/test_gpu_configs.py::test_config3_backward_batch256_vs_float64_autograd",
                                    rows="51 200 frames = 3 200 tiles on 256 workgroups x 8 waves", trips=2),
    "mcep_mfma_bwd_kernel_h": dict(test="tests/test_gpu_configs.py::test_mcep_backward_split_tail_is_bit_identical_to_whole_tiles",
                                   rows="32 768 frames and a tail = 2 048 tiles and a tail on 256 workgroups x 4 waves", trips=3),
    "frame_window_lpc24_mfma_kernel": dict(test="tests/test_gpu_lpc_fused.py::test_fused_lpc_bench_size_properties",
                                           rows="204 800 frames = 5 120 items of 40 on 768 workgroups x 4 waves", trips=2),
    "frame_window_lpc24_bwd_mfma_kernel": dict(test="tests/test_gpu_lpc_fused.py::test_fused_lpc_bench_size_properties",
                                               rows="204 800 frames = 5 120 runs of 40 hops on 2 048 one-wave workgroups", trips=3),
    "lpc24_bwd_kernel": dict(test="tests/test_gpu_parity.py::test_lpc_tuned_backward_matches_float64_path",
                             rows="70 001 frames = 1 945 items of 36 on 1 024 workgroups", trips=2),
    # ---- the 48 kHz Newton kernels (their arithmetic is out of this table's scope: classified only)
    "mcep_big_newton_kernel": dict(test="tests/test_gpu_configs.py::test_48khz_newton_steps_wide_tiles_and_plan_give_the_narrow_tiles_bits",
                                   rows="40 000 frames = 313 wide / 625 narrow tiles on 256 workgroups", trips=3),
    "mcep_big_newton4_kernel": dict(test="tests/test_gpu_configs.py::test_48khz_newton_steps_twin_workgroups_give_the_same_bits",
                                    rows="70 001 frames = 1 094 tiles on 512 workgroups", trips=3),
    "mgcep_step_h_kernel": dict(test="tests/test_gpu_configs.py::test_mgcep_whole_step_in_one_launch_against_the_two_launch_step_and_the_oracle",
                                rows="32 789 frames = 2 050 tiles on 256 workgroups x 8 waves", trips=2),
}

OUT_OF_REACH = {
    "interp_bwd_kernel": "the loop runs over the elements of gx: 2^28 float32 are 1 GiB of gx and of x, and `period` times that each of y and "
                         "its cotangent.  Period 1 is the identity (start 0; the three rows past the cap put it above 4 GiB as well); "
                         "period 2, the first that interpolates: 6 GiB",
}

# seconds per case on an MI355X as the case itself prints them (from its first line to its last assertion's figures: preparation,
# every batch, the references), one process running the whole file, when the table was written; by pytest's own count the whole
# file, imports included, took 7.3 s, which bounds every case
SECONDS = {
    "mlsacheck_tuned_kernel-mlsacheck-fwd-M3-modefast-n_fft256-f32": 0.458,
    "mlsacheck_tuned_kernel-mlsacheck-bwd-M3-modefast-n_fft256-f32": 0.718,
    "mlsacheck_tuned_kernel-mlsacheck-fwd-M3-modeclip-n_fft256-f32": 0.005,
    "mlsacheck_tuned_kernel-mlsacheck-bwd-M3-modeclip-n_fft256-f32": 0.004,
    "mlsacheck_generic_kernel-mlsacheck-fwd-M3-modefast-n_fft256-f64": 0.001,
    "mlsacheck_generic_kernel-mlsacheck-bwd-M3-modefast-n_fft256-f64": 0.002,
    "mlsacheck_generic_kernel-mlsacheck-fwd-M3-modescale-n_fft8-f32": 0.002,
    "mlsacheck_generic_kernel-mlsacheck-fwd-M3-modescale-n_fft8-f64": 0.002,
    "mlsacheck_generic_kernel-mlsacheck-bwd-M3-modescale-n_fft8-f32": 0.003,
    "mlsacheck_generic_kernel-mlsacheck-bwd-M3-modescale-n_fft8-f64": 0.003,
    "mlsacheck_generic_kernel-mlsacheck-fwd-M3-modeclip-n_fft8-f32": 0.002,
    "mlsacheck_generic_kernel-mlsacheck-fwd-M3-modeclip-n_fft8-f64": 0.002,
    "mlsacheck_generic_kernel-mlsacheck-bwd-M3-modeclip-n_fft8-f32": 0.002,
    "mlsacheck_generic_kernel-mlsacheck-bwd-M3-modeclip-n_fft8-f64": 0.002,
    "excite_kernel-excite-fwd-N5-P2-f32": 0.050,
    "excite_kernel-excite-fwd-N5-P2-f64": 0.010,
    "lsp_lpc2lsp_fwd_kernel-lpc2lsp-fwd-M2-f32": 0.036,
    "lsp_lpc2lsp_fwd_kernel-lpc2lsp-fwd-M2-f64": 0.035,
    "lsp_lpc2lsp_bwd_kernel-lpc2lsp-bwd-M2-f32": 0.037,
    "lsp_lpc2lsp_bwd_kernel-lpc2lsp-bwd-M2-f64": 0.811,
    "parcor_row_kernel-parcor-fwd-oplpc2par-M33-f32": 0.017,
    "parcor_row_kernel-parcor-fwd-oplpc2par-M33-f64": 0.014,
    "parcor_row_kernel-parcor-bwd-oplpc2par-M33-f32": 0.022,
    "parcor_row_kernel-parcor-bwd-oplpc2par-M33-f64": 0.024,
    "parcor_row_kernel-parcor-fwd-oppar2lpc-M33-f32": 0.010,
    "parcor_row_kernel-parcor-fwd-oppar2lpc-M33-f64": 0.010,
    "parcor_row_kernel-parcor-bwd-oppar2lpc-M33-f32": 0.034,
    "parcor_row_kernel-parcor-bwd-oppar2lpc-M33-f64": 0.034,
    "parcor_row_kernel-parcor-fwd-oplpccheck-M33-f32": 0.019,
    "parcor_row_kernel-parcor-fwd-oplpccheck-M33-f64": 0.019,
    "parcor_row_kernel-parcor-bwd-oplpccheck-M33-f32": 0.050,
    "parcor_row_kernel-parcor-bwd-oplpccheck-M33-f64": 0.051,
    "mcpf_fwd_kernel-mcpf-fwd-M1-alpha0.42-beta0.2-onset1-ir_length8-f32": 0.004,
    "mcpf_fwd_kernel-mcpf-fwd-M1-alpha0.42-beta0.2-onset1-ir_length8-f64": 0.003,
    "mcpf_bwd_kernel-mcpf-bwd-M1-alpha0.42-beta0.2-onset1-ir_length8-f32": 0.004,
    "mcpf_bwd_kernel-mcpf-bwd-M1-alpha0.42-beta0.2-onset1-ir_length8-f64": 0.007,
    "stft_span_gather_kernel-stft-bwd-L320-P80-nfft512-T7-f32": 0.140,
    "stft512_fwd_kernel-stft-fwd-L320-P80-nfft512-T81-f32": 0.050,
    "stft512_bwd_kernel-stft-bwd-L320-P80-nfft512-T81-f32": 0.065,
    "stft512_fwd_pk_kernel-stft-fwd-L400-P80-nfft512-T161-f32": 0.078,
    "stft512_bwd_pk_kernel-stft-bwd-L400-P80-nfft512-T161-f32": 0.099,
    "stft_big_fwd_pk_kernel-stft-fwd-L1200-P240-nfft2048-T240-f32": 0.115,
    "stft_big_bwd_pk_kernel-stft-bwd-L1200-P240-nfft2048-T240-f32": 0.149,
    "frame_window_lpc24_kernel-lpc_exact-fwd-T161-f32": 0.078,
    "griffin_update_kernel-griffin-fwd-N3-n_iter2-f32": 0.269,
    "griffin_update_kernel-griffin-fwd-N3-n_iter2-f64": 0.286,
    "div_rows_kernel-unframe-fwd-L30-P7-N3-f32": 0.003,
    "div_rows_kernel-unframe-fwd-L30-P7-N3-f64": 0.002,
    "frame_fwd_vec4_kernel-frame-fwd-L400-P80-T161-f32": 0.003,
    "window_fwd_kernel-window-fwd-L25-f32": 0.002,
    "window_fwd_kernel-window-fwd-L25-f64": 0.001,
    "window_bwd_kernel-window-bwd-L25-f32": 0.003,
    "window_bwd_kernel-window-bwd-L25-f64": 0.003,
    "window_vec4_kernel-window-fwd-L400-f32": 0.004,
    "th_solve_fwd_kernel-routes-bwd-liketh_solve_bwd-thsolve-bwd-n24-onlyf64-f64": 0.007,
    "th_solve_bwd_kernel-routes-bwd-liketh_solve_bwd-thsolve-bwd-n25-onlyf64-f64": 0.004,
    "thsolve_quad24_kernel-routes-bwd-liketh_solve_quad_bwd-thsolve-bwd-n24-onlyf32-f32": 0.004,
    "thsolve_quadn_kernel-routes-bwd-liketh_solve_quadn_bwd-thsolve-bwd-n25-onlyf32-f32": 0.004,
    "thsolve_octn_kernel-routes-bwd-liketh_solve_quadn_bwd-thsolve-bwd-n55-onlyf32-f32": 0.008,
    "mgcep_step_bwd_h_kernel-mgcep_step_h-bwd-M24-f32": 0.063,
    "matmul_rows_lds_kernel-routes-fwd-likefreqt_lds_fwd-freqt-fwd-L148-L225-f32": 0.002,
    "matmul_rows_lds_kernel-routes-fwd-likefreqt_lds_fwd-freqt-fwd-L148-L225-f64": 0.001,
    "matmul_rows_lds_kernel-routes-bwd-likefreqt_lds_bwd-freqt-bwd-L148-L225-f32": 0.002,
    "matmul_rows_lds_kernel-routes-bwd-likefreqt_lds_bwd-freqt-bwd-L148-L225-f64": 0.001,
    "fbank_bwd_kernel-routes-bwd-likefbank_bwd-fbank-bwd-nfft64-C12-use_powerTrue-gamma-0.5-f32": 0.003,
    "fbank_bwd_kernel-routes-bwd-likefbank_bwd-fbank-bwd-nfft64-C12-use_powerTrue-gamma-0.5-f64": 0.002,
    "fbank_fwd_kernel-routes-bwd-likefbank_bwd-fbank-bwd-nfft64-C12-use_powerFalse-gamma0.0-f64": 0.019,
    "fbank_mfma_fwd_kernel-routes-fwd-likefbank_mfma_fwd-fbank-fwd-nfft638-C12-use_powerFalse-gamma0.0-F5-onlyf32-f32": 0.003,
    "fbank_mfma_fwd_kernel-routes-fwd-nfft64C12use_powerTruegamma-0.5-f32": 0.001,
    "fbank_bins_bwd_kernel-routes-bwd-likefbank_bins_bwd-fbank_bins-bwd-nfft64-C12-gamma0.0-onlyf32-f32": 0.276,
    "pqmf_fwd_generic_kernel-routes-fwd-likepqmf_bwd_x-pqmf-bwd-K9-M40-T300-f32": 0.022,
    "ipqmf_fwd_generic_kernel-routes-fwd-K2M128T70-f32": 0.077,
    "ipqmf_bwd_y_kernel-routes-bwd-likeipqmf_bwd_y-ipqmf-bwd-K4-M41-T70-U3-s1-f32": 0.055,
    "interp_fwd_kernel-routes-fwd-likeinterpolate_fwd-interpolate-fwd-T7-P3-s2-f32": 0.003,
    "pqmf_bwd_x_kernel-routes-bwd-K1M7T320P16s1-f32": 0.010,
}
