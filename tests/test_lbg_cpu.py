"""VectorQuantization, InverseVectorQuantization and LindeBuzoGrayAlgorithm without a GPU: the float64 restatement the GPU tests lean on
(tests/lbg_ref.py) against the goldens of the reference (tests/golden/lbg.npz, make_golden_lbg.py) -- codebook bits and indices equal,
distances to 16 times the deviation the generator measured --, the grid the goldens have to cover, the API surface, buffers and error
texts against tests/golden/lbg_api.json, and the refusals that need no device."""
import inspect
import re

import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
import lbg_ref
from conftest import GOLDEN
from diffsptk_amd import _lib

API, CASES = lbg_ref.golden_cases(GOLDEN)
ENTRIES = {"dsa_vq_search": 12, "dsa_vq_accum_workspace_bytes": 3, "dsa_vq_accum": 8, "dsa_vq_update": 11, "dsa_vq_lookup": 8, "dsa_vq_vjp": 8}


def case_id(c):
    return (f"L{c['L']}-K{c['K']}-T{c['T']}-{c['dtype']}" + (f"-init{c['init_rows']}" if c["init_rows"] else "") + ("-repair" if c["repair"] else "")
            + (f"-{c['stops']}" if c["stops"] else "") + (f"-pf{c['perturb_factor']:g}" if c["perturb_factor"] != 1e-5 else "")
            + (f"-batch{c['batch_size']}" if c["batch_size"] else "") + (f"-warmup-{c['warmup']['var_type']}" if c["warmup"] else ""))


def test_the_goldens_cover_what_they_should():
    shapes = {(c["L"], c["K"], c["T"]) for c in CASES}
    assert shapes >= {(1, 1, 10), (2, 2, 10), (3, 4, 64), (5, 8, 257), (5, 8, 65), (25, 16, 4000), (25, 64, 4096)}
    assert all(c["T"] * c["K"] * c["L"] <= 4096 * 64 * 25 and c["T"] <= 4096 for c in CASES)
    assert {(c["init_rows"], c["K"]) for c in CASES if c["init_rows"]} >= {(1, 4), (2, 4), (3, 6), (3, 12)}
    repairs = [c for c in CASES if c["repair"]]
    assert repairs and all(c["min_data"] > 1 and max(s for per in c["n_small"] for s in per) in (1, 2) and c["dtype"] == "f32" for c in repairs)
    assert all(not any(s for per in c["n_small"] for s in per) for c in CASES if not c["repair"])
    assert any(c["stops"] == "eps" and all(n < c["n_iter"] for n in c["iterations"]) for c in CASES)
    assert any(c["stops"] == "n_iter" and all(n == c["n_iter"] for n in c["iterations"]) for c in CASES)
    assert {c["perturb_factor"] for c in CASES} >= {1e-5, 1e-2} and {c["dtype"] for c in CASES} == {"f32", "f64"}
    assert any(c["batch_size"] and c["T"] % c["batch_size"] for c in CASES)
    assert {c["warmup"]["var_type"] for c in CASES if c["warmup"]} == {"diag", "full"}
    assert all(c["gap"] >= 2.0 ** -40 for c in CASES)
    assert all(np.abs(c["x"] * 256 - np.round(c["x"] * 256)).max() == 0 and np.abs(c["x"]).max() < 8 for c in CASES)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_restatement_matches_the_reference(c):
    got = lbg_ref.run_case(c)
    assert np.array_equal(got["codebook"].view(np.int32), c["codebook"].view(np.int32))   # the bits
    assert np.array_equal(got["indices"], c["indices"]) and np.array_equal(got["n_data"], c["n_data"])
    assert got["sizes"] == c["sizes"] and [len(d) for d in got["distances"]] == c["iterations"]
    bound = 16 * max(API["restatement_deviation"], c["e_ref"])
    for mine, ref in zip(got["distances"], c["distances"]):
        assert all(abs(a - b) <= bound * max(1.0, b) for a, b in zip(mine, ref)), (mine, ref, bound)
    if c["warmup"]:
        w, mu, sigma = lbg_ref.warmup(c["x"], got["codebook"], got["indices"], lbg_ref.make_mask(c["L"], c["warmup"]["var_type"], c["warmup"]["block_size"]))
        assert np.array_equal(w, c["w"]) and np.array_equal(mu, c["mu"])
        assert np.abs(sigma - c["sigma"]).max() <= 16 * max(c["sigma_deviation"], 2.0 ** -53 * np.abs(c["x"]).max() ** 2)


def signature(f):
    return [[p.name, p.kind.name, None if p.default is inspect._empty else repr(p.default)] for p in inspect.signature(f).parameters.values()]


def test_api_surface_is_the_references():
    for cls, methods in API["signatures"].items():
        for name, want in methods.items():
            assert signature(getattr(getattr(dsp, cls), name)) == want, (cls, name)
    assert API["alias"] and dsp.LBG is dsp.LindeBuzoGrayAlgorithm and API["in_root"] == [True] * 4
    for name in ("VectorQuantization", "InverseVectorQuantization", "LindeBuzoGrayAlgorithm", "LBG"):
        assert name in dsp.__all__ and name not in dsp.modules.__all__
    assert not [n for n in dir(dsp.functional) if "vq" in n.lower() or "lbg" in n.lower()]


@pytest.mark.parametrize("name", sorted(lbg_ref.ERRORS))
def test_errors_are_the_references(name):
    with pytest.raises(Exception) as e:   # noqa: PT011
        lbg_ref.ERRORS[name](dsp)
    assert [type(e.value).__name__, str(e.value)] == API["errors"][name]


def test_buffers_and_state_dict():
    vq = dsp.VectorQuantization(2, 5)
    assert list(vq.codebook.shape) == API["codebook"]["shape"] and str(vq.codebook.dtype) == API["codebook"]["dtype"] == "torch.float32"
    assert list(vq.state_dict()) == ["codebook"] and not list(vq.parameters())
    lbg = dsp.LBG(2, 4)
    # the reference's quantiser wraps the package's module, so its key has one more level (with the generator's stand-in: vq.vq.codebook)
    assert sorted(k for k, _ in lbg.named_buffers()) == ["vq.codebook"] == [k[3:] for k in API["lbg_buffers"]] and list(lbg.state_dict()) == ["vq.codebook"]
    assert not lbg.vq.training and lbg.curr_codebook_size == 1 and dsp.LBG(2, 12).curr_codebook_size == 3
    init = torch.arange(6.0).reshape(2, 3)
    seeded = dsp.LBG(2, 8, init=init)
    assert seeded.curr_codebook_size == 2 and seeded.init == "none" and torch.equal(seeded.vq.codebook[:2], init)
    assert not list(dsp.InverseVectorQuantization().state_dict())


def test_keyword_arguments_of_the_package_are_refused():
    with pytest.raises(TypeError, match="'decay'.*vector_quantize_pytorch"):
        dsp.VectorQuantization(2, 5, decay=0.9)
    with pytest.raises(TypeError, match="'freeze_codebook'.*vector_quantize_pytorch"):
        dsp.VectorQuantization(2, 5)(torch.zeros(3), freeze_codebook=True)


def test_cpu_tensors_are_refused():
    for dtype in (torch.float32, torch.float64):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            dsp.VectorQuantization(1, 2).eval()(torch.zeros(5, 2, dtype=dtype))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            dsp.VectorQuantization(1, 2).train()(torch.zeros(5, 2, dtype=dtype))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            dsp.LBG(1, 2)(torch.zeros(5, 2, dtype=dtype))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dsp.InverseVectorQuantization()(torch.zeros(4, dtype=torch.int64), torch.zeros(3, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dsp.LBG(1, 2).transform(torch.zeros(5, 2))
    with pytest.raises(TypeError, match="float32/float64"):
        dsp.VectorQuantization(1, 2)(torch.zeros(5, 2, dtype=torch.float16))
    with pytest.raises(ValueError, match=re.escape("dimension of x must be 2")):
        dsp.VectorQuantization(1, 2)(torch.zeros(5, 3))


def test_the_ceiling_on_the_vector_length_is_refused_by_name():
    last = _lib.VQ_MAX_LENGTH
    assert last == 64 and _lib.VQ_TILE_BYTES * (last | 1) + _lib.VQ_CHUNK * last * 4 <= 160 * 1024
    for module in (dsp.VectorQuantization(last, 2), dsp.LBG(last, 2)):   # L = last + 1
        with pytest.raises(ValueError, match=f"DSA_VQ_MAX_LENGTH = {last}"):
            module(torch.zeros(3, last + 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # inside the ceiling only the device is missing
        dsp.LBG(last - 1, 2)(torch.zeros(3, last))
    lib = _lib.load()   # the library refuses by name too, before it looks at a pointer
    for rc in (lib.dsa_vq_search(None, None, 3, 2, last + 1, _lib.F32, None, None, None, None, 0.0, None),
               lib.dsa_vq_accum(None, None, 3, 2, last + 1, _lib.F64, None, None),
               lib.dsa_vq_update(None, None, 0, 3, 2, last + 1, 1, None, None, None, None)):
        assert rc == _lib.ERR_INVALID_ARGUMENT and "DSA_VQ_MAX_LENGTH (64 elements)" in lib.dsa_last_error().decode()
    assert lib.dsa_vq_accum_workspace_bytes(3, 2, last + 1) == -1 and lib.dsa_vq_accum_workspace_bytes(3, 2, last) == 2 * (last + 1) * 8


def test_a_zero_count_is_a_no_op_before_any_pointer():
    lib = _lib.load()
    assert lib.dsa_vq_search(None, None, 0, 2, 3, _lib.F32, None, None, None, None, 0.0, None) == 0
    assert lib.dsa_vq_accum(None, None, 0, 2, 3, _lib.F32, None, None) == 0
    assert lib.dsa_vq_update(None, None, 0, 0, 2, 3, 1, None, None, None, None) == 0
    assert lib.dsa_vq_lookup(None, None, 0, 2, 3, _lib.F64, None, None) == 0
    assert lib.dsa_vq_vjp(None, None, None, None, 0, _lib.F64, None, None) == 0
    assert lib.dsa_vq_search(None, None, 3, 2, 3, _lib.F32, None, None, None, None, 0.0, None) == _lib.ERR_INVALID_ARGUMENT
    assert "vq: null pointer" in lib.dsa_last_error().decode()


def test_workspace_follows_the_segments():
    lib = _lib.load()
    size = lambda T, K, L: lib.dsa_vq_accum_workspace_bytes(T, K, L)   # noqa: E731
    assert size(256, 2, 3) == 1 * 2 * 4 * 8 and size(257, 2, 3) == 2 * 2 * 4 * 8   # one vector past a segment: a second segment
    assert size(10 ** 6, 2, 3) == _lib.VQ_MAX_SEGMENTS * 2 * 4 * 8
    assert size(4096, 1000, 25) == 16 * 1000 * 26 * 8   # 1000 codewords of 25: 13 chunks of 80; 4096 waves / 52 = 79, but 4096 / 256 = 16 segments


def test_build_recipe_and_version():
    header = open(_lib.HEADER).read()
    assert int(re.search(r"#define DSA_VERSION (\d+)", header).group(1)) >= 143 and _lib.VERSION >= 143
    assert "vq.hip" in _lib.SOURCES and _lib.SOURCE_FLAGS["vq.hip"] == _lib._NO_PK
    for name, n_args in ENTRIES.items():
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name) and len(_lib.SIGNATURES[name][1]) == n_args, name
    assert _lib.load().dsa_version() >= 143
