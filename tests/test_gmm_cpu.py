"""GaussianMixtureModeling without a GPU: the float64 restatement the GPU tests lean on (tests/gmm_ref.py) against the goldens of the
reference (tests/golden/gmm.npz, make_golden_gmm.py) to 16 times the deviation the generator measured, the grid the goldens have to
cover, the API surface, buffers and error texts against tests/golden/gmm_api.json, and the refusals that need no device."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
import gmm_ref
from conftest import GOLDEN
from diffsptk_amd import _lib

CASES = gmm_ref.golden_cases(GOLDEN)
API = json.load(open(os.path.join(GOLDEN, "gmm_api.json")))


def relative(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / max(1.0, np.abs(np.asarray(want)).max()))


def test_the_goldens_cover_what_they_should():
    assert {c["L"] for c in CASES} >= {1, 2, 3, 5, 25, 50} and {c["K"] for c in CASES} >= {1, 2, 3, 8, 16}
    assert {c["T"] for c in CASES} >= {10, 63, 64, 65, 257, 1100, 4000}   # 257: one vector past a segment of the moment sums
    routes = {(c["var_type"], tuple(c["block_size"] or ())) for c in CASES}
    assert routes >= {("diag", ()), ("full", ()), ("diag", (2, 2)), ("diag", (3, 3)), ("diag", (2, 3)), ("full", (2, 3))}
    assert {(c["alpha"], gmm_ref.is_diag(c["var_type"], c["block_size"])) for c in CASES if c["alpha"]} == {(0.5, True), (1.0, True), (0.5, False), (1.0, False)}
    assert any(c.get("floors_a_weight") and c["weight_floor"] == 1 / (2 * c["K"]) for c in CASES)
    assert any(c.get("constant_column") is not None and np.all(c["sigma"][:, c["constant_column"], c["constant_column"]] == c["var_floor"]) for c in CASES)
    assert {c["n_iter"] for c in CASES} >= {1, 2, 8}
    assert any(c["n_run"] < c["n_iter"] for c in CASES) and any(c["n_run"] == c["n_iter"] == 8 for c in CASES)
    widths = {(t["Lx"], c["L"]) for c in CASES for t in c["transforms"]}
    assert {1, 2} <= {lx for lx, _ in widths} and any(lx == L // 2 and L >= 25 for lx, L in widths) and any(lx == L for lx, L in widths)
    assert sum(c["overlap"] for c in CASES) * 2 >= len(CASES)
    assert all(c["T"] * c["K"] * c["L"] <= 4000 * 25 * 16 for c in CASES)
    assert API["restatement_deviation"] * 16 <= gmm_ref.F64_BOUND <= 1e-10


@pytest.mark.parametrize("c", CASES, ids=gmm_ref.case_id)
def test_restatement_matches_the_reference(c):
    got = gmm_ref.train(c["x"], *c["init"], ubm=c["ubm"], **gmm_ref.options(c))
    assert got["n_run"] == c["n_run"] and got["mass"] >= 2.0
    worst = {q: relative(got[q][::c["post_stride"]] if q == "posterior" else got[q], c[q]) for q in gmm_ref.QUANTITIES}
    diag = gmm_ref.is_diag(c["var_type"], c["block_size"])
    params = tuple(np.asarray(c[q], dtype=np.float32).astype(np.float64) for q in ("w", "mu", "sigma"))
    for j, t in enumerate(c["transforms"]):
        y, idx, lp, gap = gmm_ref.transform(c[f"t{j}_x"].astype(np.float64), *params, diag)
        assert np.array_equal(idx, c[f"t{j}_indices"]) and gap.min() > 1e-3
        worst[f"t{j}"] = max(relative(lp, c[f"t{j}_log_prob"]), 0.0 if y is None else relative(y, c[f"t{j}_y"]))
        assert (y is None) == (t["Lx"] == c["L"])
    assert max(worst.values()) <= gmm_ref.F64_BOUND, worst


def signature(f):
    return [[p.name, p.kind.name, None if p.default is inspect._empty else repr(p.default)] for p in inspect.signature(f).parameters.values()]


def test_api_surface_is_the_references():
    cls = dsp.GaussianMixtureModeling
    for name, want in API["signatures"].items():
        assert signature(getattr(cls, name)) == want, name
    assert API["alias"] and dsp.GMM is cls and API["in_root"] == [True, True]
    assert "GaussianMixtureModeling" in dsp.__all__ and "GMM" in dsp.__all__
    assert "GaussianMixtureModeling" not in dsp.modules.__all__ and "GMM" not in dsp.modules.__all__
    assert API["functional"] == [] and not [n for n in dir(dsp.functional) if "gmm" in n.lower()]


@pytest.mark.parametrize("name", sorted(gmm_ref.ERRORS))
def test_errors_are_the_references(name):
    with pytest.raises(Exception) as e:   # noqa: PT011
        gmm_ref.ERRORS[name](dsp)
    assert [type(e.value).__name__, str(e.value)] == API["errors"][name]


def test_buffers_and_state_dict_are_the_references():
    plain = dsp.GMM(2, 3)
    ubm = dsp.GMM(2, 3, ubm=(torch.ones(3) / 3, torch.zeros(3, 3), torch.eye(3).repeat(3, 1, 1)), alpha=0.5)
    for key, m in (("plain", plain), ("ubm", ubm)):
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == API["state_dict"][key]
        assert sorted(k for k, _ in m.named_buffers()) == API["buffers"][key]
    assert torch.equal(ubm.w, ubm.ubm_w) and torch.equal(ubm.sigma, ubm.ubm_sigma)   # the background model is also the start
    state = {k: torch.full(shape, 0.5) for k, shape in API["state_dict"]["ubm"].items()}   # a state_dict of the reference's keys loads
    ubm.load_state_dict(state)
    assert float(ubm.mu[1, 1]) == 0.5 and float(ubm.ubm_sigma[2, 0, 1]) == 0.5
    assert plain.is_diag and not dsp.GMM(2, 3, var_type="full").is_diag and not dsp.GMM(3, 3, block_size=[2, 2]).is_diag
    for var_type, blocks in (("diag", None), ("full", None), ("diag", [2, 2]), ("diag", [2, 3]), ("full", [2, 3]), ("diag", [3, 3]), ("diag", [1, 2, 1])):
        L = sum(blocks) if blocks else 4
        assert np.array_equal(dsp.GMM(L - 1, 2, var_type=var_type, block_size=blocks).mask.numpy(), gmm_ref.make_mask(L, var_type, blocks))


def test_cpu_tensors_are_refused():
    for dtype in (torch.float32, torch.float64):
        gmm = dsp.GMM(1, 2, var_type="full", dtype=dtype)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            gmm(torch.zeros(5, 2, dtype=dtype))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            gmm.transform(torch.zeros(5, 1, dtype=dtype))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            gmm._e_step(torch.zeros(5, 2, dtype=dtype), reduction="none")
    with pytest.raises(RuntimeError, match="expected scalar type"):
        dsp.GMM(1, 2)(torch.zeros(5, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match=re.escape("x must be (T, 2)")):
        dsp.GMM(1, 2)(torch.zeros(5, 3))
    with pytest.raises(ValueError, match="reduction mean is not supported."):
        dsp.GMM(1, 2)._e_step(torch.zeros(5, 2), reduction="mean")


@pytest.mark.parametrize("dtype,last", [(torch.float32, 69), (torch.float64, 63)])
def test_sizes_beyond_the_lds_limit_are_refused_by_name(dtype, last):
    limit, size = _lib.GMM_MAX_LDS_BYTES, torch.empty(0, dtype=dtype).element_size()
    assert limit <= 160 * 1024
    assert dsp.ops.gmm_lds_bytes(last, size) <= limit < dsp.ops.gmm_lds_bytes(last + 1, size)
    assert dsp.ops.gmm_lds_bytes(last, size) == 2048 * (last + 1) + last * (last + 1) * size + 64
    gmm = dsp.GMM(last, 1, dtype=dtype)   # L = last + 1
    with pytest.raises(ValueError, match=f"DSA_GMM_MAX_LDS_BYTES = {limit}"):
        gmm(torch.zeros(3, last + 1, dtype=dtype))
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # inside the ceiling only the device is missing
        dsp.GMM(last - 1, 1, dtype=dtype)(torch.zeros(3, last, dtype=dtype))
    lib = _lib.load()   # the library refuses by name too, before it looks at a pointer
    code = _lib.F32 if dtype == torch.float32 else _lib.F64
    assert lib.dsa_gmm_estep(None, None, None, None, None, 3, 1, last + 1, last + 1, 0, code, None, None, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert "DSA_GMM_MAX_LDS_BYTES (163840 bytes" in lib.dsa_last_error().decode()
    assert lib.dsa_gmm_accum_workspace_bytes(3, 1, last + 1, 0, code) == -1 and lib.dsa_gmm_accum_workspace_bytes(3, 1, last, 0, code) > 0


def test_warmup_is_not_implemented():
    with pytest.raises(NotImplementedError, match="LindeBuzoGrayAlgorithm"):
        dsp.GMM(1, 2).warmup(torch.zeros(5, 2), n_iter=3)


def test_build_recipe_and_version():
    header = open(_lib.HEADER).read()
    assert int(re.search(r"#define DSA_VERSION (\d+)", header).group(1)) >= 141 and _lib.VERSION >= 141
    assert "gmm.hip" in _lib.SOURCES and _lib.SOURCE_FLAGS["gmm.hip"] == _lib._NO_PK
    for name in ("dsa_gmm_prepare", "dsa_gmm_estep", "dsa_gmm_accum", "dsa_gmm_update", "dsa_gmm_regress", "dsa_gmm_transform"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name), name
    # the moment sums' workspace: one segment per 256 vectors while the grid is short of 4096 waves, never more than 64
    ws = _lib.load().dsa_gmm_accum_workspace_bytes
    assert ws(256, 1, 5, 0, _lib.F64) == 36 * 8 and ws(257, 1, 5, 0, _lib.F64) == 2 * 36 * 8 and ws(10 ** 6, 1, 5, 0, _lib.F64) == 64 * 36 * 8
    assert ws(10 ** 6, 4096, 5, 0, _lib.F32) == 4096 * 36 * 4 and ws(10 ** 6, 512, 5, 0, _lib.F32) == 8 * 512 * 36 * 4
    assert ws(257, 3, 5, 1, _lib.F32) == 2 * 3 * 11 * 4
