"""PQMF / IPQMF / Decimation / Interpolation without a GPU: the filter design against the reference's filters
(tests/golden/pqmf.npz), the reference's signatures, errors, warning and state-dict keys (tests/golden/pqmf_api.json; both generated
by importing the reference: tests/golden/make_golden_pqmf.py), the module contract, and the C-ABI entries."""
import copy
import ctypes
import inspect
import json
import os
import pickle
import re
import warnings

import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
import diffsptk_amd.functional as F
from diffsptk_amd import _lib
from diffsptk_amd.utils import tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = json.load(open(os.path.join(ROOT, "tests", "golden", "pqmf_api.json")))
CLASSES = {"PQMF": dsp.PQMF, "IPQMF": dsp.IPQMF, "Decimation": dsp.Decimation, "Interpolation": dsp.Interpolation}
ENTRIES = ("dsa_pqmf_fwd", "dsa_pqmf_bwd", "dsa_ipqmf_fwd", "dsa_ipqmf_bwd", "dsa_interpolate_fwd", "dsa_interpolate_bwd")


def sig(f):
    return [[p.name, p.kind.name, None if p.default is inspect._empty else repr(p.default)] for p in inspect.signature(f).parameters.values()]


def test_signatures_are_the_references():
    for name, want in API["classes"].items():
        assert sig(CLASSES[name].__init__) == want["init"], name
        assert sig(CLASSES[name].forward) == want["forward"], name
    for name, want in API["functional"].items():
        assert sig(getattr(F, name)) == want, name
    for name in ("PQMF", "IPQMF", "PseudoQuadratureMirrorFilterBankAnalysis", "PseudoQuadratureMirrorFilterBankSynthesis", "Decimation",
                 "Interpolation", "FusedPQMFDecimation", "FusedInterpolationIPQMF"):
        assert name in dsp.__all__, name
    assert dsp.PQMF is dsp.PseudoQuadratureMirrorFilterBankAnalysis and dsp.IPQMF is dsp.PseudoQuadratureMirrorFilterBankSynthesis


@pytest.mark.parametrize("case", API["errors"], ids=lambda c: f"{c['kind']}-{c['module']}-{c['args']}-{c['kwargs']}")
def test_invalid_options_raise_the_references_errors(case):
    """Every case is rejected before anything reaches a device."""
    try:
        if case["kind"] == "ctor":
            CLASSES[case["module"]](*case["args"], **case["kwargs"])
        elif case["kind"] == "call":
            CLASSES[case["module"]](*case["args"], **case["kwargs"])(torch.zeros(case["shape"], dtype=torch.float64))
        else:
            getattr(F, case["module"])(torch.zeros(case["shape"], dtype=torch.float64), *case["args"], **case["kwargs"])
        got = ["ok", ""]
    except Exception as e:   # noqa: BLE001
        got = [type(e).__name__, str(e)]
    assert got == case["raises"]


def test_the_warning_is_the_references():
    for w in API["warnings"]:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            CLASSES[w["module"]](*w["args"])
        assert [str(r.message) for r in rec] == w["messages"], w


def test_filters_are_the_references(golden):
    z = golden("pqmf")
    n = 0
    for key in z.files:
        if not key.startswith("filt_"):
            continue
        _, K, M, mode, oi = key.split("_")
        h, ok = tables.pqmf_filters(int(K), int(M), mode, **API["options"][int(oi)])
        np.testing.assert_allclose(h, z[key], rtol=0, atol=1e-12, err_msg=key)
        if int(oi):
            assert ok == bool(z[f"conv_{K}_{M}_{mode}_{oi}"]), key
        n += 1
    assert n == len(API["bands"]) * len(API["filter_orders"]) * 2 + (len(API["options"]) - 1) * 4
    conv = z["converged"]
    for a, K in enumerate(API["bands"]):
        for b, M in enumerate(range(2, 64)):
            for c, mode in enumerate(("analysis", "synthesis")):
                assert tables.pqmf_filters(K, M, mode)[1] == bool(conv[a, b, c]), (K, M, mode)
    assert not conv[3, 0, 0]   # K = 4, M = 2 does not converge (the warning's case)


def test_module_filters_state_dict_pickle():
    h, _ = tables.pqmf_filters(4, 40)
    g, _ = tables.pqmf_filters(4, 40, "synthesis")
    a, s = dsp.PQMF(4, 40, dtype=torch.float64), dsp.IPQMF(4, 40, dtype=torch.float64)
    assert a.filters.shape == (4, 1, 41) and s.filters.shape == (1, 4, 41)
    assert np.array_equal(a.filters[:, 0].numpy(), h[:, ::-1]) and np.array_equal(s.filters[0].numpy(), g[:, ::-1])
    assert dsp.PQMF(4, 40).filters.dtype == torch.float32
    mods = {"PQMF": dsp.PQMF(4, 40), "PQMF_learnable": dsp.PQMF(4, 40, learnable=True), "IPQMF": dsp.IPQMF(4, 40),
            "IPQMF_learnable": dsp.IPQMF(4, 40, learnable=True)}
    for tag, m in mods.items():
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == API["state"][tag], tag
        assert isinstance(m.filters, torch.nn.Parameter) == tag.endswith("learnable")
        for m2 in (pickle.loads(pickle.dumps(m)), copy.deepcopy(m)):
            assert type(m2) is type(m) and torch.equal(m2.filters, m.filters)
    fresh = dsp.PQMF(4, 40, learnable=True)
    with torch.no_grad():
        fresh.filters.zero_()
    fresh.load_state_dict(mods["PQMF_learnable"].state_dict())
    assert torch.equal(fresh.filters, mods["PQMF_learnable"].filters)


def test_decimation_and_interpolation_contract():
    for M in (dsp.Decimation, dsp.Interpolation):
        for name in ("_func", "_check", "_precompute", "_forward"):
            assert isinstance(inspect.getattr_static(M, name), staticmethod), (M, name)
        m = M(3, start=1)
        assert m._state() == {"period": 3, "start": 1, "dim": -1} and m.state_dict() == {}
        m2 = pickle.loads(pickle.dumps(m))
        assert m2._state() == m._state() and copy.deepcopy(m)._state() == m._state()
    assert "._func(" in inspect.getsource(F.decimate) and "._func(" in inspect.getsource(F.interpolate)
    # the reference's docstring example; a view, as there
    x = torch.arange(9.0)
    y = dsp.Decimation(3, start=1)(x)
    assert y.tolist() == [1.0, 4.0, 7.0] and y._base is x
    assert torch.equal(F.decimate(x.view(3, 3), 2, 1, dim=0), x.view(3, 3)[1::2])


def test_fuse_takes_the_subband_pairs():
    a, dec, itp, s = dsp.PQMF(4, 40), dsp.Decimation(4), dsp.Interpolation(4), dsp.IPQMF(4, 40)
    assert isinstance(dsp.fuse(a, dec), dsp.FusedPQMFDecimation) and isinstance(dsp.fuse(itp, s), dsp.FusedInterpolationIPQMF)
    with pytest.raises(ValueError, match="decimate must be a Decimation"):
        dsp.fuse(a, itp)
    with pytest.raises(ValueError, match="ipqmf must be"):
        dsp.fuse(itp, a)
    with pytest.raises(ValueError, match="fuse\\(pqmf, decimate\\)"):
        dsp.fuse(a, dec, dec)


def test_the_entries_are_in_the_header_the_signatures_and_the_library():
    header = open(os.path.join(ROOT, "include", "diffsptk_amd.h")).read()
    assert int(re.search(r"#define DSA_VERSION (\d+)", header).group(1)) >= 132
    lib = ctypes.CDLL(_lib.build())
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert "pqmf.hip" in _lib.SOURCES and _lib.SOURCE_FLAGS["pqmf.hip"] == _lib._NO_PK
    # sizes are validated and a zero count is a no-op before any pointer is looked at (no device needed for either)
    L = _lib.load()
    assert L.dsa_pqmf_fwd(None, None, 0, 100, 4, 40, 1, 0, _lib.F32, None, None) == 0
    assert L.dsa_ipqmf_bwd(None, None, None, 3, 0, 4, 40, 4, 0, _lib.F64, None, None, None, None) == 0
    assert L.dsa_interpolate_fwd(None, 5, 0, 3, 2, 0, _lib.F32, None, None) == 0
    assert L.dsa_pqmf_fwd(None, None, 1, 100, 0, 40, 1, 0, _lib.F32, None, None) == -1            # K = 0
    assert L.dsa_pqmf_bwd(None, None, None, 1, 100, 4, 1, 1, 0, _lib.F32, None, None, None, None) == -1   # M = 1
    assert L.dsa_ipqmf_fwd(None, None, 1, 100, 4, 40, 0, 0, _lib.F32, None, None) == -1          # up = 0
    assert L.dsa_interpolate_bwd(None, 1, 10, 1, 2, -1, _lib.F32, None, None) == -1              # start < 0


def test_cpu_tensors_are_refused():
    """No CPU fallback: valid arguments on the host reach ops and are refused there."""
    for call in (lambda: dsp.PQMF(4, 40)(torch.zeros(100)), lambda: dsp.IPQMF(4, 40)(torch.zeros(4, 25)),
                 lambda: dsp.Interpolation(4)(torch.zeros(25)), lambda: dsp.fuse(dsp.PQMF(4, 40), dsp.Decimation(4))(torch.zeros(100))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
