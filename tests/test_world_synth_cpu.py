"""WorldSynthesis without a GPU: the conditions the goldens were generated under, re-asserted from the stored numbers
(tests/golden/make_golden_world_synth.py), the API surface, buffers and error texts against tests/golden/world_synth_api.json, the
exports, the header's section and the refusals that need no device."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
import world_synth_cases as W
from conftest import GOLDEN
from diffsptk_amd import _lib

API, Z = W.load(GOLDEN)
CASE = {c["name"]: c for c in API["cases"]}


def signature(f):
    return [[p.name, p.kind.name, None if p.default is inspect._empty else repr(p.default)] for p in inspect.signature(f).parameters.values()]


def test_the_fixtures_are_small():
    for stem in W.FILES:
        assert os.path.getsize(os.path.join(GOLDEN, stem + ".npz")) < 1 << 20   # each file; 3 MB was the budget for all of them
    assert sum(os.path.getsize(os.path.join(GOLDEN, stem + ".npz")) for stem in W.FILES) <= 3_000_000


@pytest.mark.parametrize("name", list(W.CASES))
def test_the_conditions_of_the_goldens_hold(name):
    c, rec = W.CASES[name], CASE[name]
    f0, ap, sp = W.inputs(name)
    assert np.array_equal(Z[f"{name}_f0"], f0) and f0.dtype == ap.dtype == sp.dtype == np.float32   # exact in float32 by construction
    assert np.abs(f0.astype(np.float64) - (c["sr"] / c["L"] + 1)).min() >= 1e-3
    index, index32 = Z[f"{name}_index"], Z[f"{name}_index32"]
    assert rec["pulses"] == len(index) == len(Z[f"{name}_shift"]) and rec["same_pulses"] == np.array_equal(index, index32)
    if name != "mixed_even":
        assert rec["same_pulses"] and rec["wrap_margin"] >= 1e-3 and rec["vuv_margin"] >= 1e-3
        assert 0 < rec["D_ulp_y"] < 1e-12 and rec["D_ulp_gsp"] < 1e-12 and rec["D_ulp_gap"] < 1e-12 and rec["E_ref"] > 0
    else:
        assert not rec["same_pulses"] and rec["vuv_margin"] == 0.0   # the exact tie of an even frame_period
    # the reference's batch-wide noise_size equals the per-utterance one: the first pulse of every later utterance lies before the last
    # pulse of the one before it
    for b in range(1, f0.shape[0]):
        assert index[index[:, 0] == b][0, 1] <= index[index[:, 0] == b - 1][-1, 1]
    assert np.all(np.diff(index[:, 0]) >= 0) and all(np.all(np.diff(index[index[:, 0] == b][:, 1]) > 0) for b in range(f0.shape[0]))
    shift = Z[f"{name}_shift"] * c["sr"]
    assert np.all((shift >= 0) & (shift <= 1))
    # the noise the tests inject is the noise the generator recorded
    assert float(np.abs(W.noise(name, rec["pulses"], c["L"]).astype(np.float64)).sum()) == rec["noise_sum"]
    T = f0.shape[1] * c["P"]
    assert Z[f"{name}_y"].shape[-1] == c.get("out_length", T) and Z[f"{name}_gsp"].shape[-2:] == sp.shape[-2:]


def test_the_cases_cover_what_they_are_for():
    _, ap, sp = W.inputs("mixed_odd")
    assert (ap == 0).any() and (ap == 1).any() and (sp == 0).any() and ((sp > 0) & (sp < W.EPS)).any()
    f0 = W.inputs("mixed_odd")[0]
    assert ((f0 > 0) & (f0 < 16000 / 1024 + 1)).sum() == 1
    assert W.CASES["mixed_odd"]["P"] % 2 == 1 and W.CASES["mixed_even"]["P"] % 2 == 0
    assert CASE["sparse"]["max_noise_size"] > W.CASES["sparse"]["L"] and CASE["sparse"]["pulses"] == 3
    assert int(np.log2(W.CASES["wide"]["L"])) % 2 == 1   # the lone last stage of the LDS transform
    assert not W.CASES["unbatched"]["batched"] and W.CASES["unbatched"]["out_length"] < 8 * 75
    assert API["no_pulse"] == "RuntimeError"


def test_api_surface_is_the_references():
    for name, want in API["signatures"].items():
        assert signature(getattr(dsp.WorldSynthesis, name)) == want, name
    assert API["in_root"] and "WorldSynthesis" in dsp.__all__ and "WorldSynthesis" not in dsp.modules.__all__
    assert not API["has_functional"] and not hasattr(dsp.functional, "world_synth")


@pytest.mark.parametrize("name", sorted(W.ERRORS))
def test_errors_are_the_references(name):
    with pytest.raises(Exception) as e:   # noqa: PT011
        W.ERRORS[name](dsp)
    assert [type(e.value).__name__, str(e.value)] == API["errors"][name]


def test_buffers_and_state_dict_are_the_references():
    for key, dtype in (("float32", None), ("float64", torch.float64)):
        m = dsp.WorldSynthesis(80, 16000, 1024, dtype=dtype)
        assert {k: [str(v.dtype), list(v.shape)] for k, v in m.named_buffers()} == API["buffers"][key]
        assert sorted(m.state_dict()) == API["state_dict"] == []
        assert torch.equal(m.ramp, torch.arange(1024))
        assert np.array_equal(m.dc_remover.numpy(), Z["dc_remover64" if dtype else "dc_remover32"])


def test_build_recipe_version_and_header():
    header = open(_lib.HEADER).read()
    assert int(re.search(r"#define DSA_VERSION (\d+)", header).group(1)) >= 144 and _lib.VERSION >= 144
    assert "world_synth.hip" in _lib.SOURCES and _lib.SOURCE_FLAGS["world_synth.hip"] == _lib._NO_PK
    for name in ("dsa_world_synth_pulses", "dsa_world_synth_responses", "dsa_world_synth_overlap_add", "dsa_world_synth_vjp_pulses",
                 "dsa_world_synth_vjp_frames"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name), name
    assert re.search(r"a24\s+WORLD synthesis", header) and "world_synth.py:166-321" in header and "common.py:73-84, 141-163" in header
    assert re.search(r"#define DSA_WORLD_LDS_BYTES\(L, size\) \(\(4 \* \(L\) \+ 4\) \* \(size\) \+ 256\)", header)
    assert _lib.WORLD_MAX_LDS_BYTES == 163840


@pytest.mark.parametrize("dtype,last", [(torch.float32, 8192), (torch.float64, 4096)])
def test_lengths_outside_the_limits_are_refused_by_name(dtype, last):
    size = torch.empty(0, dtype=dtype).element_size()
    assert all(dsp.ops.world_lds_bytes(L, size) == (4 * L + 4) * size + 256 for L in (1024, 2048, 4096, 8192, 16384))
    assert dsp.ops.world_lds_bytes(4096, 8) <= _lib.WORLD_MAX_LDS_BYTES and dsp.ops.world_lds_bytes(4096, 4) <= _lib.WORLD_MAX_LDS_BYTES
    assert dsp.ops.world_lds_bytes(last, size) <= _lib.WORLD_MAX_LDS_BYTES < dsp.ops.world_lds_bytes(2 * last, size)
    with pytest.raises(ValueError, match=f"DSA_WORLD_MAX_LDS_BYTES = {_lib.WORLD_MAX_LDS_BYTES}"):   # the first size outside, before any device
        dsp.WorldSynthesis(80, 16000, 2 * last, dtype=dtype)
    with pytest.raises(ValueError, match="power of two.*DSA_WORLD_MAX_LDS_BYTES"):
        dsp.WorldSynthesis(80, 16000, 1536, dtype=dtype)
    m = dsp.WorldSynthesis(80, 16000, last, dtype=dtype)   # the last size inside: only the device is missing
    D = last // 2 + 1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, dtype=dtype), torch.zeros(2, D, dtype=dtype), torch.ones(2, D, dtype=dtype))
    if dtype == torch.float64:   # a float32 module at 8192 takes float64 data no further than the limit of float64
        with pytest.raises(ValueError, match="DSA_WORLD_MAX_LDS_BYTES"):
            dsp.WorldSynthesis(80, 16000, 8192)(torch.zeros(2, dtype=dtype), torch.zeros(2, 4097, dtype=dtype), torch.ones(2, 4097, dtype=dtype))
    lib = _lib.load()   # the library refuses by name too, before it looks at a pointer
    code = _lib.F32 if dtype == torch.float32 else _lib.F64
    assert lib.dsa_world_synth_pulses(None, 1, 4, 80, 16000, 2 * last, 500.0, None, code, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert "world_synth" in lib.dsa_last_error().decode() and "DSA_WORLD_MAX_LDS_BYTES (163840 bytes" in lib.dsa_last_error().decode()
    assert lib.dsa_world_synth_pulses(None, 1, 4, 80, 16000, 1536, 500.0, None, code, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert "world_synth: fft_length must be a power of two" in lib.dsa_last_error().decode()
    assert lib.dsa_world_synth_pulses(None, 1, 4, 80, 16000, last, 500.0, None, code, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.dsa_last_error().decode() == "world_synth: null pointer"   # inside the ceiling only the pointers are missing
    for B, N, pulses in ((0, 4, 3), (1, 0, 3), (1, 4, 0)):   # a zero count is a no-op before any pointer is looked at
        assert lib.dsa_world_synth_responses(None, None, None, None, None, None, None, None, B, N, 16000, last, pulses, code, None, None) == 0
        assert lib.dsa_world_synth_vjp_pulses(None, None, None, None, None, None, None, None, None, B, N, 100, 16000, last, pulses, code, None, None) == 0
    assert lib.dsa_world_synth_pulses(None, 0, 4, 80, 16000, last, 500.0, None, code, None, None, None, None) == 0
    assert lib.dsa_world_synth_overlap_add(None, None, None, 0, 100, last, 0, code, None, None) == 0
    assert lib.dsa_world_synth_vjp_frames(None, None, None, None, None, None, 0, 4, last, 0, code, None, None, None) == 0


def test_a_bin_count_other_than_half_the_transform_is_refused():
    with pytest.raises(ValueError, match=r"fft_length / 2 \+ 1 = 513 bins"):
        dsp.WorldSynthesis(80, 16000, 1024)(torch.zeros(2), torch.zeros(2, 512), torch.ones(2, 512))
    with pytest.raises(RuntimeError, match="expected scalar type"):
        dsp.WorldSynthesis(80, 16000, 1024)(torch.zeros(2, dtype=torch.float64), torch.zeros(2, 513, dtype=torch.float64),
                                            torch.ones(2, 513, dtype=torch.float64))
