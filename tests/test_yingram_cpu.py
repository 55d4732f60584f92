"""Yingram without a GPU: the API surface, buffers, tables and error texts against tests/golden/yingram_api.json and yingram.npz
(make_golden_yingram.py), the float64 restatement the GPU tests lean on (tests/yingram_ref.py) against the goldens to 16 times the
deviation the generator measured, its gradient against central differences, the two departures from the reference (a ValueError at
construction where the reference's forward raises IndexError; a finite value at an integral lag), and the refusals that need no
device."""
import inspect
import re

import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
import yingram_ref as R
from conftest import GOLDEN
from diffsptk_amd import _lib

API, CASES = R.golden_cases(GOLDEN)
F64_BOUND = 16 * API["restatement_deviation"]


def module_tables(c):
    """(lags, floor, ceil, lag_max) as a float64 module of the package holds them"""
    m = dsp.Yingram(c["L"], dtype=torch.float64, **R.options(c))
    return m.lags.numpy(), m.lags_floor.numpy(), m.lags_ceil.numpy(), len(m.ramp) + 1


def relative(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / max(1.0, np.abs(np.asarray(want)).max()))


def signature(f):
    return [[p.name, p.kind.name, None if p.default is inspect._empty else repr(p.default)] for p in inspect.signature(f).parameters.values()]


def test_the_goldens_cover_the_grid():
    names = {c["name"] for c in CASES}
    assert names == {f"L{g[0]}_{kind}" for g in R.GRID for kind in ("noise", "voiced")} | {"silent", "fused_center1", "fused_center0"}
    for c in CASES:
        assert np.array_equal(c["x"], c["x"].astype(np.float32)) and np.array_equal(c["gy"], c["gy"].astype(np.float32))   # exact in float32
        assert c["dev_y"] <= 1e-10 and c["dev_g"] <= 1e-10
    assert 0 < F64_BOUND <= 1e-10 and all(ret == "IndexError" for ret, _ in API["index_errors"])
    lengths = {c["L"] for c in CASES}   # frames on both sides of the length at which AUTO changes the route
    assert min(lengths) < _lib.YINGRAM_FFT_MIN_FRAME_LENGTH <= max(lengths)


def test_api_surface_is_the_references():
    for name, want in API["signatures"].items():
        assert signature(getattr(dsp.Yingram, name)) == want, name
    assert signature(dsp.functional.yingram) == API["functional"]
    assert API["in_root"] and "Yingram" in dsp.__all__ and "Yingram" not in dsp.modules.__all__


@pytest.mark.parametrize("name", sorted(R.ERRORS))
def test_errors_are_the_references(name):
    with pytest.raises(Exception) as e:   # noqa: PT011
        R.ERRORS[name](dsp)
    assert [type(e.value).__name__, str(e.value)] == API["errors"][name]


def test_buffers_and_state_dict_are_the_references():
    for key, dtype in (("float32", None), ("float64", torch.float64)):
        m = dsp.Yingram(64, dtype=dtype)
        assert {k: str(v.dtype) for k, v in m.named_buffers()} == API["buffers"][key]
        assert sorted(m.state_dict()) == API["state_dict"] == []


@pytest.mark.parametrize("key", sorted(API["tables"]))
def test_tables_are_the_references(key):
    t, z = dict(API["tables"][key]), R.golden_tables(GOLDEN, key)
    L, M = t.pop("L"), t.pop("M")
    for dtype, lags in ((torch.float64, z["lags64"]), (torch.float32, z["lags32"])):
        m = dsp.Yingram(L, dtype=dtype, **t)
        assert m.lags.dtype == dtype and np.array_equal(m.lags.numpy(), lags) and len(m.lags) == M
        assert np.array_equal(m.lags_floor.numpy(), z["floor"]) and np.array_equal(m.lags_ceil.numpy(), z["ceil"])
        assert torch.equal(m.ramp, torch.arange(1, t["lag_max"] or L - 1))
    lags, floor, ceil, K = R.tables(L, **t)   # the restatement's own construction: the same bins, the lags to a few units in the last place
    assert np.array_equal(floor, z["floor"]) and np.array_equal(ceil, z["ceil"]) and K == (t["lag_max"] or L - 1)
    assert np.abs(lags / z["lags64"] - 1).max() <= 16 * 2.0 ** -52


@pytest.mark.parametrize("c", CASES, ids=R.case_id)
def test_restatement_matches_the_reference(c):
    tables = module_tables(c)   # the restatement on the package's own tables
    assert tables[3] == c["K"]
    x = c["x"] if c["frame"] is None else R.frames(c["x"], c["L"], *c["frame"])
    y = R.forward(x, *tables)
    g = R.gradient(x, c["gy"], *tables)
    if c["frame"] is not None:
        g = R.unframe_adjoint(g, len(c["x"]), c["L"], *c["frame"])
    dy, dg = relative(y, c["y"]), relative(g, c["gx"])
    print(f"{c['name']}: y {dy:.3g}, gradient {dg:.3g}, bound {F64_BOUND:.3g}")
    assert dy <= F64_BOUND and dg <= F64_BOUND
    if c["kind"] == "silent":
        assert not y.any() and np.isfinite(g).all()


def test_restatement_gradient_matches_central_differences():
    c = next(c for c in CASES if c["name"] == "L32_noise")
    args = module_tables(c)
    x, gy = c["x"][:1], c["gy"][:1]
    g = R.gradient(x, gy, *args)
    h = 1e-6
    numeric = np.zeros_like(x)
    for i in range(x.shape[-1]):
        e = np.zeros_like(x)
        e[0, i] = h
        numeric[0, i] = ((R.forward(x + e, *args) - R.forward(x - e, *args)) * gy).sum() / (2 * h)
    # a central difference of step h on a smooth function: O(h^2) truncation and rounding of 2^-52 |y| / h, both far below 1e-7
    assert relative(g, numeric) <= 1e-7


def test_index_errors_of_the_reference_are_value_errors_at_construction():
    for kw in R.INDEX_ERRORS:
        with pytest.raises(ValueError, match=r"The largest lag, .* lag_max - 1 = ") as e:
            dsp.Yingram(**kw)
        assert f"lag_max = {kw.get('lag_max', kw['frame_length'] - 1)}" in str(e.value)
        with pytest.raises(ValueError):
            R.tables(kw["frame_length"], kw["sample_rate"], kw["lag_min"], kw.get("lag_max"), 20)


def test_an_integral_lag_returns_the_limit():
    o = dict(R.INTEGRAL)
    L = o.pop("L")
    lags, floor, ceil, K = R.tables(L, **o)
    whole = np.flatnonzero(floor == ceil)
    assert len(whole) >= 1 and 20 in floor[whole]
    x = np.random.default_rng(5).normal(size=(2, L))
    y = R.forward(x, lags, floor, ceil, K)
    dn, _ = R.normalised(R.difference(x, K))
    assert np.isfinite(y).all() and np.array_equal(y[:, whole], dn[:, floor[whole]])
    gy = np.zeros_like(y)
    gy[:, whole[0]] = 1.0   # its gradient is that of d'[lag] alone
    only = R.gradient(x, gy, lags, floor, ceil, K)
    assert np.isfinite(only).all() and np.abs(only).max() > 0
    m = dsp.Yingram(L, dtype=torch.float64, **o)
    assert np.array_equal(m.lags_floor.numpy(), floor) and np.array_equal(m.lags_ceil.numpy(), ceil)


def test_cpu_tensors_are_refused():
    for dtype in (torch.float32, torch.float64):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            dsp.Yingram(64, dtype=dtype)(torch.zeros(3, 64, dtype=dtype))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            dsp.functional.yingram(torch.zeros(3, 64, dtype=dtype))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dsp.fuse(dsp.Frame(64, 16), dsp.Yingram(64))(torch.zeros(200))
    with pytest.raises(RuntimeError, match="expected scalar type"):
        dsp.Yingram(64)(torch.zeros(3, 64, dtype=torch.float64))


def test_fuse_takes_a_frame_and_a_yingram_of_one_length():
    assert isinstance(dsp.fuse(dsp.Frame(64, 16), dsp.Yingram(64)), torch.nn.Module)
    with pytest.raises(ValueError, match="frame and yingram disagree on frame_length."):
        dsp.fuse(dsp.Frame(32, 16), dsp.Yingram(64))
    with pytest.raises(ValueError, match=re.escape("fuse(frame, yingram) takes a Frame and a Yingram, and no options.")):
        dsp.fuse(dsp.Frame(64, 16), dsp.Yingram(64), exact_lag_sums=True)
    with pytest.raises(ValueError, match=re.escape("fuse(frame, window, lpc) takes a Frame, a Window and a LinearPredictiveCodingAnalysis.")):
        dsp.fuse(dsp.Frame(4, 2), dsp.Window(4))


def test_build_recipe_and_version():
    header = open(_lib.HEADER).read()
    assert int(re.search(r"#define DSA_VERSION (\d+)", header).group(1)) >= 142 and _lib.VERSION >= 142
    assert "yingram.hip" in _lib.SOURCES and _lib.SOURCE_FLAGS["yingram.hip"] == _lib._NO_PK
    for name in ("dsa_yingram", "dsa_yingram_vjp", "dsa_frame_yingram"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name), name
    assert re.search(r"#define DSA_YINGRAM_LDS_BYTES\(H, L, size\) \(\(3 \* \(H\) \+ 1\) \* \(size\) \+ 8 \* \(\(L\) \+ 1\) \+ 128\)", header)
    assert _lib.YINGRAM_FFT_MIN_FRAME_LENGTH >= 2


def formula(L, size):
    """DSA_YINGRAM_LDS_BYTES at the half length H of the longest lag range: 2 H the power of two from 2 L - 1 on"""
    H = 2
    while 2 * H < 2 * L - 1:
        H *= 2
    return (3 * H + 1) * size + 8 * (L + 1) + 128


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_sizes_beyond_the_lds_limit_are_refused_by_name(dtype):
    limit, size = _lib.YINGRAM_MAX_LDS_BYTES, torch.empty(0, dtype=dtype).element_size()
    assert limit <= 160 * 1024 and dsp.ops.yingram_lds_bytes(4096, size) <= limit
    last = max(L for L in range(4096, 16386) if formula(L, size) <= limit)   # the formula says where the ceiling is
    assert all(dsp.ops.yingram_lds_bytes(L, size) == formula(L, size) for L in (2, 3, 32, 400, 2048, 4096, 4097, last, last + 1))
    assert dsp.ops.yingram_lds_bytes(last, size) <= limit < dsp.ops.yingram_lds_bytes(last + 1, size)
    with pytest.raises(ValueError, match=f"DSA_YINGRAM_MAX_LDS_BYTES = {limit}"):
        dsp.Yingram(last + 1, dtype=dtype)(torch.zeros(1, last + 1, dtype=dtype))
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # inside the ceiling only the device is missing
        dsp.Yingram(last, dtype=dtype)(torch.zeros(1, last, dtype=dtype))
    lib = _lib.load()   # the library refuses by name too, before it looks at a pointer
    code = _lib.F32 if dtype == torch.float32 else _lib.F64
    for algo in (_lib.ALGO_AUTO, _lib.ALGO_GENERIC, _lib.ALGO_TUNED):
        assert lib.dsa_yingram(None, 3, last + 1, last, None, None, None, 5, None, algo, code, None, None) == _lib.ERR_INVALID_ARGUMENT
        assert "DSA_YINGRAM_MAX_LDS_BYTES (163840 bytes" in lib.dsa_last_error().decode()
    assert lib.dsa_yingram_vjp(None, None, 3, last + 1, last, None, None, None, 5, None, 0, code, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert "DSA_YINGRAM_MAX_LDS_BYTES" in lib.dsa_last_error().decode()
    assert lib.dsa_frame_yingram(None, 1, 100, last + 1, 10, 1, last, None, None, None, 5, None, 0, code, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert "DSA_YINGRAM_MAX_LDS_BYTES" in lib.dsa_last_error().decode()
    assert lib.dsa_yingram(None, 3, last, last - 1, None, None, None, 5, None, 0, code, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.dsa_last_error().decode() == "yingram: null pointer"   # inside the ceiling only the pointers are missing
    assert lib.dsa_yingram(None, 0, last, last - 1, None, None, None, 5, None, 0, code, None, None) == 0   # an empty batch is a no-op
