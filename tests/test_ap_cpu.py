"""Aperiodicity without a GPU: the conditions the goldens were generated under, re-asserted from the stored numbers
(tests/golden/make_golden_ap.py), the restatement (tests/ap_ref.py) against the reference's goldens, its integers and its gradient, the
API surface, buffers and error texts against tests/golden/ap_api.json, the departures that need no device, the ceiling and the build
recipe."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ap_cases as A
import ap_ref
import diffsptk_amd as dsp
from conftest import GOLDEN
from diffsptk_amd import _lib, ops

API, Z = A.load(GOLDEN)
CASE = {c["name"]: c for c in API["cases"]}
MEASURED = [n for n in A.CASES if n != A.SILENT]


def signature(f):
    return [[p.name, p.kind.name, None if p.default is inspect._empty else repr(p.default)] for p in inspect.signature(f).parameters.values()]


def restate(name, dtype=np.float64, with_grad=True):
    (P, sr, L), kw = A.module_args(name)
    kw = dict(kw)
    fmt = A.FORMATS[kw.pop("out_format")]
    detail = {}
    gy = A.cotangent(name, Z[f"{name}_y"].shape) if with_grad else None
    out = ap_ref.aperiodicity(Z[f"{name}_x"], Z[f"{name}_f0"], P, sr, L, out_format=fmt, gy=gy, dtype=dtype, detail=detail, **kw)
    dec = np.stack([np.stack([f.t0, f.bias, np.broadcast_to(f.cpos, f.t0.shape)]) for f in detail["fits"]])
    return out, dec, detail["fits"]


def test_the_fixtures_are_small():
    assert os.path.getsize(os.path.join(GOLDEN, "ap.npz")) < 1 << 20 and os.path.getsize(os.path.join(GOLDEN, "ap_api.json")) < 1 << 20


@pytest.mark.parametrize("name", list(A.CASES))
def test_the_conditions_of_the_goldens_hold(name):
    rec = CASE[name]
    x, f0 = A.inputs(name)
    assert np.array_equal(Z[f"{name}_x"], x) and np.array_equal(Z[f"{name}_f0"], f0) and x.dtype == f0.dtype == np.float32
    assert x.shape[1] == A.CASES[name].get("T", 12 * A.CASES[name]["P"]) and np.array_equal(x * 4096, np.round(x * 4096))
    assert rec["margin"] == A.half_integer_margin(name) >= 1e-3   # every pitch + 0.5 and pitch / 2 + 0.5 stays 1e-3 from an integer
    assert (f0 <= 32).any() and (f0 >= 997).any()
    assert rec["n_band"] == ops.ap_bands(rec["sr"])[0] == Z[f"{name}_int64"].shape[0]
    if name != A.SILENT:   # cholesky_ex succeeded at the first trial in both dtypes: one call per band
        assert rec["cholesky64"] == rec["cholesky32"] == rec["n_band"]
        assert 0 < rec["D_ulp"] < 1e-11 and rec["restatement_deviation"] < 1e-11 and rec["E_ref"] > 0 and rec["E_gref"] > 0
    assert rec["same_decisions"] == np.array_equal(Z[f"{name}_int64"], Z[f"{name}_int32"])


def test_the_cases_cover_what_they_are_for():
    segs = {J for sr in A.GROUPS for J in ops.ap_bands(sr)[2]}
    assert segs == {46, 61, 91, 121, 181, 241, 361, 721}   # J < 64, and ragged last strides of the 64 lanes
    assert A.CASES["ties8k"]["P"] % 2 == 1
    cpos = np.arange(12) * 25 * 2000 / 8000 + 1.5   # exact integers before the truncation, in the deep bands of the ties case
    assert (cpos == np.round(cpos)).sum() >= 3
    assert A.CASES["shortest"]["T"] == ops.ap_min_length(16000) == 81 and API["shortest_accepted_16k"] == [False, True]
    assert A.CASES["batched"]["N"] * A.CASES["batched"]["P"] != Z["batched_x"].shape[1] and Z["batched_f0"].shape[0] == 3
    assert len({tuple(r) for r in Z["batched_f0"]}) == 3
    assert {A.CASES[n].get("fmt") for n in ("fmt_a", "fmt_p", "fmt_ap", "fmt_pa")} == set(A.FORMATS)
    assert (Z["silent_x"] == 0).sum() >= 760 and CASE[A.SILENT]["reference_nan_y"] > 0   # the reference: NaN from log 0


def test_api_surface_is_the_references():
    for name, want in API["signatures"].items():
        assert signature(getattr(dsp.Aperiodicity, name)) == want, name
    assert API["in_root"] and "Aperiodicity" in dsp.__all__ and "Aperiodicity" not in dsp.modules.__all__
    assert not API["in_functional"] and not hasattr(dsp.functional, "ap") and not hasattr(dsp.functional, "aperiodicity")


@pytest.mark.parametrize("name", sorted(A.ERRORS))
def test_errors_are_the_references(name):
    with pytest.raises(Exception) as e:   # noqa: PT011
        A.ERRORS[name](dsp)
    assert [type(e.value).__name__, str(e.value)] == API["errors"][name]


def test_buffers_and_state_dict_are_the_references():
    for key, dtype in (("float32", None), ("float64", torch.float64)):
        for tag, L in (("bins", 64), ("bands", None)):
            m = dsp.Aperiodicity(80, 16000, L, dtype=dtype)
            assert {k: [str(v.dtype), list(v.shape)] for k, v in m.named_buffers()} == API["buffers"][f"{key}_{tag}"]
            assert sorted(m.state_dict()) == API["state_dict"] == []
        m = dsp.Aperiodicity(80, 16000, 64, dtype=dtype)
        for k in ("interp_indices", "interp_weights", "eye", "hHP", "hLP", "window"):   # casts of float64 tables: the same bits everywhere
            assert np.array_equal(getattr(m.extractor, k).numpy(), Z[f"buffer_{key}_{k}"]), (key, k)
        # the square root is taken in the module's dtype by whatever CPU runs this: one unit in the last place of room
        got, ref = m.extractor.window_sqrt.double().numpy(), Z[f"buffer_{key}_window_sqrt"].astype(np.float64)
        assert np.all(np.abs(got - ref) <= (2.0**-52 if dtype else 2.0**-23) * ref)
        assert torch.equal(m.extractor.ramp, torch.arange(-1, 242).view(1, 1, -1))


@pytest.mark.parametrize("name", MEASURED)
def test_the_restatement_matches_the_reference(name):
    rec = CASE[name]
    (y, gx), dec, fits = restate(name)
    assert np.array_equal(dec, Z[f"{name}_int64"])
    assert all(f.ok.all() and (f.trial == 0).all() for f in fits)
    lim = 16 * max(rec["restatement_deviation"], rec["D_ulp"])
    for key, got in (("y", y), ("gx", gx)):
        ref = Z[f"{name}_{key}"]
        err = float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))
        print(f"{name} {key}: {err:.3g}, bound {lim:.3g}")
        assert got.shape == ref.shape and err <= lim


@pytest.mark.parametrize("name", list(A.CASES))
def test_the_restatements_integers_are_the_references_in_both_dtypes(name):
    for dtype, key in ((np.float64, "int64"), (np.float32, "int32")):
        _, dec, _ = restate(name, dtype, with_grad=False)
        assert np.array_equal(dec, Z[f"{name}_{key}"]), (name, key)


def test_the_restatement_on_the_silent_case():
    (y, gx), _, fits = restate(A.SILENT)
    ref = Z["silent_y"]
    nan = np.isnan(ref)
    assert nan.sum() == CASE[A.SILENT]["reference_nan_y"] and any((f.A == 0).any() for f in fits)
    assert np.isfinite(y).all() and np.isfinite(gx).all() and np.all(y[nan] == 0.001)   # the bins a silent band reaches: lower_bound
    assert np.abs(y[~nan] - ref[~nan]).max() <= 1e-12


def test_the_restatements_gradient_against_central_differences():
    name = "band8k"
    (P, sr, L), kw = A.module_args(name)
    x, f0 = Z[f"{name}_x"].astype(np.float64), Z[f"{name}_f0"]
    gy = A.cotangent(name, Z[f"{name}_y"].shape).astype(np.float64)
    y, gx = ap_ref.aperiodicity(x, f0, P, sr, L, gy=gy)
    assert ((y > 0.001) & (y < 0.999)).all()   # no bin at a bound: the function is smooth here
    rng = np.random.default_rng(3)
    for _ in range(3):
        v = rng.standard_normal(x.shape)
        h = 1e-6
        fd = float(((ap_ref.aperiodicity(x + h * v, f0, P, sr, L) - ap_ref.aperiodicity(x - h * v, f0, P, sr, L)) * gy).sum() / (2 * h))
        an = float((gx * v).sum())
        # the difference quotient's own error: rounding 2^-52 |y . gy| / h ~ 1e-9, truncation h^2 f''' ~ 1e-9: 1e-6 of the value, with room
        print(f"directional derivative {an:.9g}, central difference {fd:.9g}")
        assert abs(fd - an) <= 1e-6 * max(1.0, abs(an))


def test_the_restatement_escalates_and_recovers():
    """the CPU twin of tests/test_gpu_ap.py::test_fits_that_escalate_and_recover"""
    c = A.ESCALATING
    x, f0 = A.escalating_inputs()
    gy = A.cotangent("band8k", (1, c["N"], 5)).astype(np.float64)
    detail = {}
    y, gx = ap_ref.aperiodicity(x, f0, c["P"], c["sr"], None, lower=c["lower"], eps=c["eps"], gy=gy, detail=detail)
    trials = np.stack([f.trial for f in detail["fits"]])
    print("trials per band:", [sorted({int(t) for t in band.ravel()}) for band in trials])
    assert all(f.ok.all() for f in detail["fits"]) and (trials > 0).any() and (trials == 0).any() and trials.max() < ap_ref.TRIALS
    assert np.isfinite(y).all() and np.isfinite(gx).all() and y.max() > 0.5   # values that a wrong factor would move: not all near 0
    # held to its own trials the restatement repeats itself bit for bit; held to others it does not
    y2, gx2 = ap_ref.aperiodicity(x, f0, c["P"], c["sr"], None, lower=c["lower"], eps=c["eps"], gy=gy, trials=trials)
    assert np.array_equal(y2, y) and np.array_equal(gx2, gx)
    y3 = ap_ref.aperiodicity(x, f0, c["P"], c["sr"], None, lower=c["lower"], eps=c["eps"], trials=np.full_like(trials, 8))
    assert np.isfinite(y3).all() and not np.array_equal(y3, y)
    # with the default eps nothing escalates
    ap_ref.aperiodicity(x, f0, c["P"], c["sr"], None, lower=c["lower"], detail=detail)
    assert all((f.trial == 0).all() for f in detail["fits"])
    d_y, d_g = A.escalating_sensitivity(ap_ref, x, f0, gy, trials)
    print(f"one unit in the last place of x moves y by {d_y:.3g} and gx by {d_g:.3g}")
    assert 0 < d_y < 1e-4 and 0 < d_g   # (the gradient is ill-conditioned here: |gx| reaches 1e6 where A is rounding noise)


def test_departures_that_need_no_device():
    with pytest.raises(ValueError, match="d4c is not built.*only the tandem algorithm") as e:
        dsp.Aperiodicity(80, 16000, 64, algorithm="d4c")
    assert "not supported" not in str(e.value)
    for sr, shortest in ((8000, 41), (16000, 81), (48000, 321)):
        assert ops.ap_min_length(sr) == shortest
        m = dsp.Aperiodicity(80, sr, 64)
        with pytest.raises(ValueError, match=f"at least {shortest} samples for sample_rate {sr}"):
            m(torch.zeros(1, shortest - 1), torch.zeros(1, 2))
        with pytest.raises(RuntimeError, match="no CPU fallback"):   # the shortest admissible length: only the device is missing
            m(torch.zeros(1, shortest), torch.zeros(1, 2))
    with pytest.raises(ValueError, match="x and f0 must have the same batch size"):
        dsp.Aperiodicity(80, 16000, 64)(torch.zeros(2, 960), torch.zeros(3, 12))
    with pytest.raises(RuntimeError, match="expected scalar type"):
        dsp.Aperiodicity(80, 16000, 64)(torch.zeros(2, 960, dtype=torch.float64), torch.zeros(2, 12, dtype=torch.float64))


def test_cpu_tensors_are_refused():
    for L in (64, None):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            dsp.Aperiodicity(80, 16000, L)(torch.zeros(960), torch.zeros(12))


def test_segments_beyond_the_ceiling_are_refused_by_name():
    limit = _lib.AP_MAX_LDS_BYTES
    assert limit == 163840 and _lib.AP_MAX_BANDS == 8
    n_band, _, seg = ops.ap_bands(96000)
    assert (n_band, seg) == (7, [1441, 721, 361, 181, 91, 46, 46]) and ops.ap_lds_bytes(sum(seg), n_band) == 116168 <= limit
    dsp.Aperiodicity(480, 96000, 2048)   # 96 kHz with the default window is inside
    need = lambda w: ops.ap_lds_bytes(sum(ops.ap_bands(48000, w)[2]), 6)   # noqa: E731
    last = max(w for w in range(30, 200) if need(w) <= limit)
    assert need(last) <= limit < need(last + 1)
    with pytest.raises(ValueError, match=f"DSA_AP_LDS_BYTES = {need(last + 1)} bytes.*DSA_AP_MAX_LDS_BYTES = {limit}"):
        dsp.Aperiodicity(240, 48000, 2048, window_length_ms=last + 1)
    m = dsp.Aperiodicity(240, 48000, 2048, window_length_ms=last)   # the last shape inside: only the device is missing
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 2880), torch.zeros(1, 12))
    with pytest.raises(ValueError, match="DSA_AP_MAX_BANDS = 8"):
        dsp.Aperiodicity(80, 600 * 2**9, 64)
    lib = _lib.load()   # the library refuses by name too, before it looks at a pointer
    for code in (_lib.F32, _lib.F64):
        def tandem(B, w, ldb=1 << 20):
            return lib.dsa_ap_tandem(None, ldb, None, None, None, 1 << 20, None, None, B, 12, 2880, 240, 48000, float(w), 7, 1e-5, 0.001, 0.999, 0,
                                     code, None, None)

        def tandem_vjp(B, w):
            return lib.dsa_ap_tandem_vjp(None, None, 1 << 20, None, None, None, 1 << 20, None, None, B, 12, 2880, 240, 48000, float(w), 7, 1e-5, 0.001,
                                         0.999, 0, code, None, None, None, 1 << 20, None)

        for call in (tandem, tandem_vjp):
            assert call(1, last + 1) == _lib.ERR_INVALID_ARGUMENT
            assert "ap: DSA_AP_LDS_BYTES" in lib.dsa_last_error().decode() and "DSA_AP_MAX_LDS_BYTES (163840 bytes" in lib.dsa_last_error().decode()
            assert call(1, last) == _lib.ERR_INVALID_ARGUMENT and lib.dsa_last_error().decode() == "ap: null pointer"
            assert call(0, last) == 0   # an empty batch is a no-op before any pointer is looked at
        assert tandem(1, 30, 10) == _lib.ERR_INVALID_ARGUMENT and "do not fit their rows" in lib.dsa_last_error().decode()
        assert tandem(1, 1e-4) == _lib.ERR_INVALID_ARGUMENT and lib.dsa_last_error().decode() == "ap: window_length_ms gives a segment shorter than 2 samples"
        assert tandem(1, 1e9) == _lib.ERR_INVALID_ARGUMENT and "DSA_AP_MAX_LDS_BYTES" in lib.dsa_last_error().decode()
        assert "shorter than" not in lib.dsa_last_error().decode()   # each cause has its own text
        assert lib.dsa_ap_qmf(None, 0, 100, 100, code, None, 50, None, 50, None) == 0
        assert lib.dsa_ap_qmf_vjp(None, 50, None, 50, 0, 100, code, None, 100, None) == 0
        assert lib.dsa_ap_qmf(None, 1, 20, 20, code, None, 10, None, 10, None) == _lib.ERR_INVALID_ARGUMENT
        assert "at least 21 samples" in lib.dsa_last_error().decode()
        assert lib.dsa_ap_qmf(None, 1, 21, 21, code, None, 11, None, 11, None) == _lib.ERR_INVALID_ARGUMENT
        assert lib.dsa_last_error().decode() == "ap: null pointer"
    assert lib.dsa_ap_qmf(None, 1, 21, 21, 7, None, 11, None, 11, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.dsa_last_error().decode() == "ap: unknown dtype"


def test_build_recipe_version_and_header():
    header = open(_lib.HEADER).read()
    assert int(re.search(r"#define DSA_VERSION (\d+)", header).group(1)) >= 146 and _lib.VERSION >= 146
    assert "ap.hip" in _lib.SOURCES and _lib.SOURCE_FLAGS["ap.hip"] == _lib._NO_PK
    for name in ("dsa_ap_qmf", "dsa_ap_qmf_vjp", "dsa_ap_tandem", "dsa_ap_tandem_vjp"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name), name
    assert re.search(r"a25\s+Band aperiodicity by TANDEM-STRAIGHT", header) and "ap.py:294-374" in header
    assert re.search(r"#define DSA_AP_LDS_BYTES\(S, n_band\) \(40 \* \(\(S\) \+ 2 \* \(n_band\)\) \+ 128\)", header)
    for tag in ("ap_qmf_f32", "ap_qmf_vjp_f32", "ap_tandem_f32", "ap_tandem_vjp_f32"):
        assert f'"{tag}"' in header and f'"{tag}"' in open(os.path.join(_lib.CSRC, "ap.hip")).read()
