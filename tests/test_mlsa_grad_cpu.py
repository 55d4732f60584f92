"""The MLSA gradient fixture (tests/golden/mlsa_grad.npz and mlsa_grad.json, written by tests/golden/make_golden_mlsa_grad.py from the
reference) checked on its own, so that a mistake in the generator cannot pass as a kernel bug in tests/test_gpu_mlsa_grad.py.  CPU only.

  coverage   the case list holds exactly the sets the GPU test is meant to run; every array and every E_ref is finite, E_ref > 0;
  forward    the numpy oracle (oracle.mlsa / oracle.mlsa_mixed) reproduces every stored y within 1e-8 of its maximum, the bound
             tests/test_oracle_golden.py holds this oracle to;
  gradient   for every case of sets C and D and every third case of A and B, the central difference of the oracle's (y * gy).sum()
             along one seeded random direction (dx, dmc) at h = 1e-6 equals <gx, dx> + <gmc, dmc> of the fixture within 1e-6
             relative: the truncation error is O(h^2) and rounding about 1e-16 / h, two orders below the bound."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "mlsa_grad.json")))["cases"]
MODES = ("multi-stage", "single-stage", "freq-domain")
FD = [c for c in CASES if c["set"] in "CD"] + [c for c in CASES if c["set"] in "AB"][::3]


def oracle_forward(case, x, mc):
    kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in case["kwargs"].items()}
    gamma = 0.0 if case["c"] == 0 else -1.0 / case["c"]
    if case["phase"] == "mixed":
        return O.mlsa_mixed(x, mc, case["P"], tuple(case["filter_order"]), alpha=case["alpha"], gamma=gamma,
                            ignore_gain=case["ignore_gain"], mode=case["mode"], **kw)
    return O.mlsa(x, mc, case["P"], case["alpha"], gamma, case["ignore_gain"], case["phase"], case["mode"], **kw)


def key(c):
    return (c["mode"], c["phase"], c["ignore_gain"], c["c"])


def test_the_case_list_covers_what_it_must(golden):
    g = golden("mlsa_grad")
    tags = [c["tag"] for c in CASES]
    assert len(set(tags)) == len(tags)
    by = {s: [c for c in CASES if c["set"] == s] for s in "ABCDE"}
    assert sum(len(v) for v in by.values()) == len(CASES)
    small = {"multi-stage": {"taylor_order": 7, "cep_order": 100}, "single-stage": {"ir_length": 200, "n_fft": 512},
             "freq-domain": {"frame_length": 400, "fft_length": 512}}
    # A: every mode x phase x ignore_gain at c = 0, the minimum-phase rows again at c = 2, and the non-packed STFT backward
    hamming = [c for c in by["A"] if c["kwargs"].get("window") == "hamming"]
    grid = [c for c in by["A"] if c not in hamming]
    assert {key(c) for c in grid} == ({(m, p, ig, 0) for m in MODES for p in ("minimum", "maximum", "zero") for ig in (False, True)}
                                      | {(m, "minimum", ig, 2) for m in MODES for ig in (False, True)})
    assert len(grid) == 24 and all(c["kwargs"] == small[c["mode"]] for c in grid)
    assert len(hamming) == 1 and hamming[0]["kwargs"] == {"frame_length": 512, "fft_length": 512, "window": "hamming"}
    assert hamming[0]["mode"] == "freq-domain" and hamming[0]["phase"] == "minimum"
    assert all(c["filter_order"] == 24 and c["P"] == 80 and c["alpha"] == 0.42 and g[c["x"]].shape == (960,) for c in by["A"])
    # B: mixed phase, unequal orders and pairs
    mixed = {"multi-stage": {"taylor_order": 7, "cep_order": [40, 60]}, "single-stage": {"ir_length": [80, 120], "n_fft": 512},
             "freq-domain": {"frame_length": 400, "fft_length": 512}}
    assert {key(c) for c in by["B"] if c["c"] == 0} == {(m, "mixed", ig, 0) for m in MODES for ig in (False, True)}
    assert len([c for c in by["B"] if c["c"] == 2]) == 1 and len(by["B"]) == 7
    assert all(c["filter_order"] == [12, 24] and c["kwargs"] == mixed[c["mode"]] and c["phase"] == "mixed" for c in by["B"])
    assert all(g[c["mc"]].shape == (12, 37) for c in by["B"])
    # C: the module's defaults -- no keyword arguments
    assert {(c["mode"], c["phase"]) for c in by["C"]} == {("single-stage", "minimum"), ("single-stage", "zero"), ("single-stage", "mixed"),
                                                          ("multi-stage", "minimum"), ("multi-stage", "zero")}
    assert len(by["C"]) == 5 and all(c["kwargs"] == {} and c["c"] == 0 and not c["ignore_gain"] and c["P"] == 80 for c in by["C"])
    # D: short filters at a frame period that is no multiple of four
    assert {(c["mode"], c["phase"]) for c in by["D"]} == {(m, p) for m in MODES for p in ("minimum", "zero")} and len(by["D"]) == 6
    for c in by["D"]:
        assert c["filter_order"] == 8 and c["P"] == 10 and c["alpha"] == 0 and c["c"] == 0 and g[c["mc"]].shape == (20, 9)
        assert "cep_order" not in c["kwargs"] and c["kwargs"].get("ir_length", 0) < 16
        if c["mode"] == "freq-domain":
            assert c["kwargs"] == {"frame_length": 32, "fft_length": 64}
    # E: two batch dimensions
    assert len(by["E"]) == 1 and by["E"][0]["mode"] == "multi-stage" and g[by["E"][0]["x"]].shape == (2, 2, 960)
    assert g[by["E"][0]["mc"]].shape == (2, 2, 12, 25)
    # both values of c with their own cepstra; the fixture holds nothing but the cases' arrays
    assert {c["c"] for c in CASES} == {0, 2} and not np.array_equal(g["mc_c0"], g["mc_c2"])
    names = {c[k] for c in CASES for k in ("x", "mc", "gy")} | {f"{c['tag']}_{q}" for c in CASES for q in ("y", "gx", "gmc")}
    assert set(g.files) == names
    for name in g.files:
        assert g[name].dtype == np.float64 and np.isfinite(g[name]).all(), name
    for c in CASES:
        assert g[c["tag"] + "_y"].shape == g[c["x"]].shape == g[c["tag"] + "_gx"].shape == g[c["gy"]].shape
        assert g[c["tag"] + "_gmc"].shape == g[c["mc"]].shape
        assert set(c["E_ref"]) == {"y", "gx", "gmc"}
        for q, e in c["E_ref"].items():
            assert np.isfinite(e) and 0 < e < 1e-3, (c["tag"], q, e)
    # the fixture is a committed file: 1 MB at the most
    assert os.path.getsize(os.path.join(HERE, "golden", "mlsa_grad.npz")) <= 1000000


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["tag"])
def test_the_oracle_reproduces_the_forward(golden, case):
    g = golden("mlsa_grad")
    ref = g[case["tag"] + "_y"]
    err = np.abs(oracle_forward(case, g[case["x"]], g[case["mc"]]) - ref).max() / np.abs(ref).max()
    print(f"{case['tag']}: max|oracle - ref| / max|ref| = {err:.3g}")
    assert err < 1e-8


@pytest.mark.parametrize("case", FD, ids=lambda c: c["tag"])
def test_the_gradient_along_a_random_direction(golden, case):
    g = golden("mlsa_grad")
    x, mc, gy = g[case["x"]], g[case["mc"]], g[case["gy"]]
    rng = np.random.default_rng(CASES.index(case))
    dx, dmc = rng.standard_normal(x.shape), rng.standard_normal(mc.shape)
    h = 1e-6
    f = lambda s: float((oracle_forward(case, x + s * dx, mc + s * dmc) * gy).sum())   # noqa: E731
    fd = (f(h) - f(-h)) / (2 * h)
    want = float((g[case["tag"] + "_gx"] * dx).sum() + (g[case["tag"] + "_gmc"] * dmc).sum())
    print(f"{case['tag']}: central difference {fd:.9g}, fixture {want:.9g}, relative {abs(fd - want) / abs(want):.3g}")
    assert abs(fd - want) <= 1e-6 * abs(want)
