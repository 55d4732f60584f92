"""PitchAdaptiveSpectralAnalysis without a GPU: the float64 restatement (tests/pitch_spec_ref.py) against the reference's goldens, the
fixtures' tie margins, the module's surface against what the reference's has (tests/golden/pitch_spec_api.json), the C header's section,
the two ceilings, the refusals, and what the registry tests of the library demand of the new unit, read as text."""
import ast
import inspect
import os
import re

import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
import pitch_spec_cases as A
import pitch_spec_ref
from conftest import GOLDEN
from diffsptk_amd import _lib, ops
from diffsptk_amd.modules.pitch_spec import SpectrumExtractionByCheapTrick

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API, Z = A.load(GOLDEN)
CASE = {c["name"]: c for c in API["cases"]}
UNIT = open(os.path.join(ROOT, "diffsptk_amd", "csrc", "pitch_spec.hip")).read()
ROUTES = [f"pitch_spec{kind}_{tag}" for kind in ("", "_vjp_frames", "_vjp_gather") for tag in ("f32", "f64")]


def rel(a, ref):
    return float(np.abs(a - ref).max() / max(1.0, np.abs(ref).max()))


def test_the_goldens_hold_every_case_and_stay_small():
    assert set(CASE) == set(A.CASES) == {n for names in A.FILES.values() for n in names}
    for file in list(A.FILES) + ["pitch_spec_api.json"]:
        assert os.path.getsize(os.path.join(GOLDEN, file)) < 1 << 20, file
    for name in A.CASES:
        B, N, T, L, K = A.sizes(name)
        shape = ((N, K), (T,)) if A.CASES[name].get("unbatched") else ((B, N, K), (B, T))
        assert (Z[f"{name}_y"].shape, Z[f"{name}_gx"].shape) == shape and Z[f"{name}_y"].dtype == np.float64
        assert np.isfinite(Z[f"{name}_y"]).all() and np.isfinite(Z[f"{name}_gx"]).all() and np.abs(Z[f"{name}_gx"]).max() > 0
        assert N == (T - 1) // A.CASES[name]["P"] + 1
    assert A.sizes("short")[2] < A.CASES["short"]["L"] // 2   # every frame of `short` is mostly padding
    # the reference's float32 run is finite on the first five sample-rate rows, and about 1e-3 off its float64 run at worst
    assert all(CASE[n]["E_ref"] is not None and 0 < CASE[n]["E_ref"] < 1e-2 and 0 < CASE[n]["E_gref"] < 1e-2 for n in A.FIVE_RATES)


@pytest.mark.parametrize("name", list(A.CASES))
def test_the_restatement_against_the_goldens(name):
    """within the bound the float64 kernel is held to, 64 max(D_ulp, B_dep, 2^-53); the generator's own figure is in the JSON"""
    x, f0 = A.inputs(name)
    n1, n2 = A.noises(name)
    (P, sr, L), kw = A.module_args(name)
    fmt = kw.pop("out_format")
    y, gx = pitch_spec_ref.pitch_spec(x, f0, P, sr, L, out_format=fmt, noise1=n1, noise2=n2, noise_eps=float(np.finfo(np.float64).eps),
                                      gy=A.cotangent(name).astype(np.float64), **kw)
    y, gx = A.squeeze(name, y, gx)
    lim = 64 * max(CASE[name]["D_ulp"], CASE[name]["B_dep"], 2.0 ** -53)
    err = max(rel(y, Z[f"{name}_y"]), rel(gx, Z[f"{name}_gx"]))
    print(f"{name}: {err:.3g} (stored: {CASE[name]['restatement_deviation']:.3g}), bound {lim:.3g}")
    assert err <= lim


def test_the_restatements_gradient_is_the_derivative():
    """the closed form against central differences of the restatement itself, on a few samples of a short case with the floor on"""
    name = "options"
    x, f0 = A.inputs(name)
    x, f0 = x[:1, :480].astype(np.float64), f0[:1, :6]
    (P, sr, L), kw = A.module_args(name)
    kw.pop("out_format")
    gy = A.cotangent(name)[:1, :6].astype(np.float64)
    run = lambda v: pitch_spec_ref.pitch_spec(v, f0, P, sr, L, out_format=1, gy=gy, **kw)  # noqa: E731
    _, gx = run(x)
    for t in (0, 7, 240, 479):
        d = np.zeros_like(x)
        d[0, t] = 1e-6
        num = ((run(x + d)[0] - run(x - d)[0]) * gy).sum() / 2e-6
        assert abs(num - gx[0, t]) <= 1e-5 * max(1.0, abs(gx[0, t])), (t, num, gx[0, t])


def test_the_tie_margins():
    for name in A.CASES:
        c = CASE[name]
        assert (c["margin_window"], c["margin_f_min"], c["margin_bin"]) == pytest.approx(A.margins(name), rel=1e-9), name
        assert min(c["margin_window"], c["margin_f_min"], c["margin_bin"]) >= A.MARGIN, name
    # the exception kept on purpose: the default 500 Hz is an exact multiple of sr / L at 16 kHz and at 8 kHz, where `<` is exactly false
    assert 500 / (16000 / 1024) == 32 and 500 / (8000 / 1024) == 64
    _, f0 = A.inputs("k16")
    assert (f0 <= 3 * 16000 / 1021).any() and (f0 > 3 * 16000 / 1021).any()


@pytest.mark.parametrize("name", list(A.EDGE_CASES))
def test_the_edge_cases_keep_their_margins_and_a_bound_that_says_something(name):
    """the cases below 1024 points and up to Nyquist (tests/test_gpu_pitch_spec_edges.py runs the kernels on them): what they are meant
    to reach, the three tie margins, and -- so that 64 D_ulp cannot go vacuous -- a finite restatement whose float64 bounds are at most
    1e-10, for y and gx and for the frames' cotangents, in both modes"""
    B, N, T, L, K = A.edge_sizes(name)
    c = A.EDGE_CASES[name]
    sr, P = c["sr"], c["P"]
    x, f0 = A.edge_inputs(name)
    assert (B, N) == (2, 7) and x.shape == (2, T) and f0.shape == (2, 7) and T == N * P and N == (T - 1) // P + 1
    assert np.array_equal(np.round(f0.astype(np.float64) * 8), f0.astype(np.float64) * 8) and f0.max() <= 0.49 * sr
    assert min(A.edge_margins(name)) >= A.MARGIN, A.edge_margins(name)
    assert (sr / 4) / (sr / L) == L // 4   # the default F0 is a bin exactly: `k rate < f` is exactly false there in every precision
    f_min = 3 * sr / (L - 3)
    f = np.where(f0 <= f_min, sr / 4, f0.astype(np.float64))
    assert (f0 <= f_min).any() and (f0 > f_min).sum() >= 4 and (name != "L16" or (f0 <= f_min).sum() >= 4)
    # near Nyquist the DC mask covers nearly every bin and the mirror is a third of the spectrum; just above f_min the window is widest
    consts = [pitch_spec_ref.frame_constants(float(v), sr, L) for v in f.flatten()]
    top = pitch_spec_ref.frame_constants(float(f.max()), sr, L)
    assert top[1] >= 0.43 * L and top[3] >= 0.32 * L and all(0 <= t[0] <= L // 2 - 1 and t[3] <= K - 1 and t[6] + 1 <= 2 * t[3] for t in consts)
    assert max(t[0] for t in consts) >= 0.8 * (L // 2 - 1)
    for mode in A.EDGE_MODES:
        r = A.edge_reference(name, mode)
        assert r["y"].shape == (B, N, K) and r["gx"].shape == (B, T) and r["cot"].shape == (B, N, L)
        assert all(np.isfinite(r[k]).all() and np.abs(r[k]).max() > 0 for k in ("y", "gx", "cot"))
        print(f"{name} {mode}: D_ulp {r['D_ulp']:.3g} (bound {r['bound']:.3g}), on the frames' cotangents {r['D_cot']:.3g} (bound {r['bound_cot']:.3g})")
        assert 64 * 2.0 ** -53 <= r["bound"] <= 1e-10 and 64 * 2.0 ** -53 <= r["bound_cot"] <= 1e-10
        # the helper returns what pitch_spec() adds into gx: the clipped scatter-add of the rows is gx to the bit
        gx = np.zeros((B, T))
        for b in range(B):
            for n in range(N):
                np.add.at(gx[b], np.clip(n * P + np.arange(L) - L // 2, 0, T - 1), r["cot"][b, n])
        assert np.array_equal(gx, r["gx"])


def test_the_edge_cases_cover_the_workgroup_size():
    """256 threads: L / 4 butterflies, K bins and L samples below it (16, 64), L at it (256), K above it (512), L / 4 at it (1024)"""
    assert [c["L"] for c in A.EDGE_CASES.values()] == [16, 64, 256, 512, 1024]
    assert re.search(r"constexpr int PS_THREADS = 256;", UNIT) and "L >= 16" in UNIT


def signature(f):
    return [[p.name, p.kind.name, None if p.default is inspect._empty else repr(p.default)] for p in inspect.signature(f).parameters.values()]


def test_the_surface_is_the_references():
    cls = dsp.PitchAdaptiveSpectralAnalysis
    want = API["signatures"]
    assert signature(cls.__init__) == want["__init__"] and signature(cls.forward) == want["forward"]
    assert signature(SpectrumExtractionByCheapTrick.__init__) == want["extractor.__init__"]
    assert signature(SpectrumExtractionByCheapTrick.forward) == want["extractor.forward"]
    for key, dtype in (("float32", None), ("float64", torch.float64)):
        m = cls(80, 16000, 1024, dtype=dtype)
        assert {k: [str(v.dtype), list(v.shape)] for k, v in m.named_buffers()} == API["buffers"][key]
        assert torch.equal(m.extractor.ramp, torch.arange(1024, dtype=m.extractor.ramp.dtype))
    assert sorted(cls(80, 16000, 1024).state_dict()) == API["state_dict"] == []
    e = cls(80, 16000, 1024, eps=1e-6, relative_floor=-60).extractor
    assert {k: repr(getattr(e, k)) for k in API["attributes"]} == API["attributes"]
    assert type(e.spec).__name__ == API["spec_class"] == "Spectrum" and isinstance(e.spec, dsp.Spectrum)
    assert API["in_root"] and hasattr(dsp, "PitchAdaptiveSpectralAnalysis") and "PitchAdaptiveSpectralAnalysis" in dsp.__all__
    from diffsptk_amd import functional, modules

    assert "PitchAdaptiveSpectralAnalysis" not in modules.__all__   # (modules/mlsacheck.py says why)
    assert not API["in_functional"] and not any("pitch_spec" in n for n in dir(functional))
    assert ops.PitchSpecFn is ops.pitch_spec.PitchSpecFn and issubclass(ops.PitchSpecFn, torch.autograd.Function)
    for fmt, code in (("db", 0), ("log-magnitude", 1), ("magnitude", 2), ("power", 3), (0, 0), (1, 1), (2, 2), (3, 3)):
        assert cls(80, 16000, 1024, out_format=fmt).out_format == code


@pytest.mark.parametrize("name", list(A.ERRORS))
def test_the_errors_are_the_references(name):
    want = API["errors"][name]
    try:
        A.ERRORS[name](dsp)
        got = None
    except Exception as e:  # noqa: BLE001
        got = [type(e).__name__, str(e)]
    assert got == want


def test_the_refusals_of_its_own():
    cls = dsp.PitchAdaptiveSpectralAnalysis
    with pytest.raises(ValueError, match="algorithm straight is not built: diffsptk_amd has only the cheap-trick algorithm"):
        cls(80, 16000, 1024, algorithm="straight")
    with pytest.raises(ValueError, match=r"fft_length 1536 is not a power of two"):
        cls(80, 16000, 1536)
    m = cls(80, 16000, 1024)
    with pytest.raises(ValueError, match=r"f0 must have \(T - 1\) // frame_period \+ 1 = 12 frames for a waveform of 960 samples, got 11"):
        m(torch.zeros(2, 960), torch.zeros(2, 11))
    with pytest.raises(ValueError, match="same leading dimensions"):
        m(torch.zeros(2, 960), torch.zeros(12))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 960), torch.zeros(2, 12))


def test_the_two_ceilings():
    """L = 4096 (96 kHz) is accepted; the first power of two that does not fit is refused by the constant's name, before a device is needed"""
    assert _lib.PITCH_SPEC_MAX_LDS_BYTES == 163840
    assert ops.pitch_spec_lds_bytes(4096) == 28 * 4096 + 280 <= _lib.PITCH_SPEC_MAX_LDS_BYTES < ops.pitch_spec_lds_bytes(8192)
    dsp.PitchAdaptiveSpectralAnalysis(480, 96000, 4096)
    with pytest.raises(ValueError, match=r"fft_length 8192 takes DSA_PITCH_SPEC_LDS_BYTES = 229656 bytes.*DSA_PITCH_SPEC_MAX_LDS_BYTES = 163840"):
        dsp.PitchAdaptiveSpectralAnalysis(480, 96000, 8192)
    # the library's own check, without a launch: a null pointer is refused after the sizes are accepted, the ceiling before
    lib = _lib.load()
    args = lambda L: (None, None, None, None, None, 1, 3, 1440, 480, 96000, L, 500.0, -0.15, 0.0, 0.0, 3, _lib.F32, None, None)  # noqa: E731
    assert lib.dsa_pitch_spec(*args(4096)) == _lib.ERR_INVALID_ARGUMENT and lib.dsa_last_error().decode() == "pitch_spec: null pointer"
    assert lib.dsa_pitch_spec(*args(8192)) == _lib.ERR_INVALID_ARGUMENT
    assert "DSA_PITCH_SPEC_LDS_BYTES(fft_length) = 28 fft_length + 280 bytes exceed DSA_PITCH_SPEC_MAX_LDS_BYTES" in lib.dsa_last_error().decode()
    assert lib.dsa_pitch_spec(*args(3000)) == _lib.ERR_INVALID_ARGUMENT and "power of two" in lib.dsa_last_error().decode()
    # the batch is the grid's y: 65535 utterances pass the sizes (and stop at the null pointer), 65536 are refused before any pointer
    gather = lambda B: lib.dsa_pitch_spec_vjp_gather(None, B, 3, 5, 2, 16, _lib.F64, None, None)  # noqa: E731
    assert gather(65535) == _lib.ERR_INVALID_ARGUMENT and lib.dsa_last_error().decode() == "pitch_spec: null pointer"
    assert gather(65536) == _lib.ERR_INVALID_ARGUMENT
    assert lib.dsa_last_error().decode() == "pitch_spec: invalid sizes (B N frames must fit one grid dimension)"
    small = (None, None, None, None, None, 65536, 3, 5, 2, 256, 16, 64.0, -0.15, 0.0, 0.0, 3, _lib.F64, None, None)
    assert lib.dsa_pitch_spec(*small) == _lib.ERR_INVALID_ARGUMENT
    assert lib.dsa_last_error().decode() == "pitch_spec: invalid sizes (B N frames must fit one grid dimension)"


def test_the_header_has_the_section():
    header = open(_lib.HEADER).read()
    assert int(re.search(r"#define DSA_VERSION (\d+)", header).group(1)) >= 148 and _lib.VERSION >= 148
    assert re.search(r"a26\s+Pitch-adaptive spectral envelope", header)
    assert re.search(r"T = 1 \(one frame\): the padding clamps all L columns to the one sample, and gx is their sum", header)   # 148
    for name, n_args in (("dsa_pitch_spec", 19), ("dsa_pitch_spec_vjp_frames", 20), ("dsa_pitch_spec_vjp_gather", 9)):
        assert re.search(rf"\bint {name}\(", header) and name in _lib.SIGNATURES and hasattr(_lib.load(), name), name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
    assert re.search(r"#define DSA_PITCH_SPEC_MAX_LDS_BYTES 163840\b", header) and re.search(r"#define DSA_PITCH_SPEC_LDS_BYTES\(L\)", header)
    assert "pitch_spec.hip" in _lib.SOURCES and "pitch_spec.hip" in _lib.SOURCE_FLAGS


def test_an_unknown_dtype_and_a_zero_count():
    lib = _lib.load()
    none = (None,) * 5
    tail = (80, 16000, 1024, 500.0, -0.15, 0.0, 0.0, 3)
    assert lib.dsa_pitch_spec(*none, 2, 12, 960, *tail, 99, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.dsa_last_error().decode() == "pitch_spec: unknown dtype"
    assert lib.dsa_pitch_spec_vjp_gather(None, 2, 12, 960, 80, 1024, 99, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.dsa_last_error().decode() == "pitch_spec: unknown dtype"
    for B, N, T in ((0, 12, 960), (2, 0, 0)):   # a no-op before any pointer is looked at
        assert lib.dsa_pitch_spec(*none, B, N, T, *tail, _lib.F64, None, None) == 0
        assert lib.dsa_pitch_spec_vjp_frames(None, *none, B, N, T, *tail, _lib.F64, None, None) == 0
        assert lib.dsa_pitch_spec_vjp_gather(None, B, N, T, 80, 1024, _lib.F64, None, None) == 0
    assert lib.dsa_pitch_spec(*none, 2, 11, 960, *tail, _lib.F64, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert "frames" in lib.dsa_last_error().decode()


def code_of(text):
    """the text without its // comments"""
    return re.sub(r"//[^\n]*", "", text)


def test_the_unit_fits_in():
    """what tests/test_routes_cpu.py, test_grid_strides_cpu.py, test_alignment_cpu.py, test_dtype_refusals_cpu.py and
    test_host_cpu.py::test_shared_device_helpers_are_not_copied demand of a unit, on pitch_spec.hip as text"""
    entries = [n for n in _lib.SIGNATURES if n.startswith("dsa_pitch_spec")]
    assert sorted(entries) == ["dsa_pitch_spec", "dsa_pitch_spec_vjp_frames", "dsa_pitch_spec_vjp_gather"]
    assert not any(re.fullmatch(r"dsa_\w+_(fwd|bwd)", n) for n in entries)                       # 1 no entry asks for a row of the alignment sweep
    from diffsptk_amd import modules

    assert "PitchAdaptiveSpectralAnalysis" not in modules.__all__                               # 2
    assert "gridDim." not in UNIT                                                                # 3 every grid is sized exactly
    assert "DSA_ERR_UNSUPPORTED" not in code_of(UNIT)                                            # 4 refusals are invalid arguments
    assert 'fail(DSA_ERR_INVALID_ARGUMENT, "pitch_spec: unknown dtype")' in UNIT                 # 5 the dtype refusal is the unit's own ...
    assert UNIT.index('"pitch_spec: unknown dtype"') < UNIT.index("with_dtype(")
    calls = re.findall(r"\bwith_dtype\(\s*\w+\s*,\s*([^,]+),", UNIT)
    assert calls and all(re.fullmatch(r"\w+", c.strip()) for c in calls)                        # ... and with_dtype gets the name in a variable
    assert "unsupported dtype" not in UNIT
    assert "launch_lds<" in UNIT and "hipFuncAttributeMaxDynamicSharedMemorySize" not in UNIT and "ensure_dynamic_lds" not in UNIT   # 6
    assert not re.search(r"__builtin_amdgcn_readlane|__[fd](?:mul|add|sub|div)_rn\b|\b__brev\b", UNIT) and "fft_brev(" in UNIT
    assert "atomic" not in code_of(UNIT).lower()
    # 7 the route names: spelled once each, outside every check_launch(...) and outside any k...Routes / k...Names table
    import test_routes_cpu as RC

    assert not set(ROUTES) & RC.launch_names(UNIT) and not RC.name_tables(UNIT)
    assert all(UNIT.count(f'"{r}"') == 1 for r in ROUTES)
    assert RC.launch_arguments(UNIT) == ["route)"] and len(re.findall(r"\bps_launch<", UNIT)) == 2 and UNIT.count("int ps_launch(") == 1
    assert re.search(r"int ps_launch\(const char\* route\b[^{]*\{[^}]*check_launch\(route\)", UNIT)
    import kernel_routes as KR

    # the six names are registered: pinned by the test that calls the three entries, and forwarded from the entry that spells each
    assert all(KR.PINNED_ELSEWHERE[r] == "tests/test_gpu_pitch_spec.py::test_every_launch_names_its_kernel" for r in ROUTES)
    assert all(KR.FORWARDED[r] == "csrc/pitch_spec.hip::dsa_" + r[:-4] for r in ROUTES)
    assert not set(ROUTES) & (set(KR.ROUTES) | set(KR.EXEMPT))
    assert RC.argument_problems({"pitch_spec.hip": UNIT}, KR.FORWARDED) == []


def test_every_route_name_is_pinned_by_a_gpu_test_that_reads_last_kernel():
    import test_routes_cpu as RC

    src = open(os.path.join(ROOT, "tests", "test_gpu_pitch_spec.py")).read()
    defs = {n.name: ast.get_source_segment(src, n) for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    for route in ROUTES:
        where = [name for name, body in defs.items() if f'"{route}"' in body and RC.reads_last_kernel(src, name)]
        assert where, f"no test function of tests/test_gpu_pitch_spec.py spells \"{route}\" and reads last_kernel()"


def test_the_documents_name_the_operator():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^### 3\.21 `pitch_spec\.hip`", design, re.M) and "PINNED_ELSEWHERE" in design[design.index("### 3.21"):]
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "PitchAdaptiveSpectralAnalysis(" in readme
