#!/usr/bin/env python3
"""Golden fixtures of mlsacheck, by importing the REFERENCE.  Build container only.

    python tests/golden/make_golden_mlsacheck.py     # writes tests/golden/mlsacheck.npz and mlsacheck_api.json (data)

Per case (lsp_api.json style: the list of cases with their options is in mlsacheck_api.json) the input `<tag>_x` in float64 (every value
exact in float32), and the reference's results: `<tag>_64` is [out, grad, w] in float64 and `<tag>_32` is [out, grad] in float32, grad
being the gradient of sum(w * out).

Inputs: 0.5 * randn(rows, M + 1) * linspace(1, 0.05, M + 1), each row then scaled (and, in fast mode, given the sign) so that its
amplitude a -- the plain sum of the gain-free cepstrum in fast mode, the largest spectral amplitude otherwise -- is a chosen multiple of
the threshold: every third row 1.3 .. 3 times the threshold (the check moves it), the others 0.2 .. 0.8 times (it must not).

Conditions, asserted here for every case with M >= 1 in float64 AND on the float32-rounded input (the seed is advanced until they hold;
nothing is filtered at test time):
  * the case has moved and unmoved frames;
  * |a - thr| >= 1e-3 thr in every frame;
  * clip mode: | |C_k| - thr | >= 1e-3 thr for every bin of every frame;
  * scale mode: in a moved frame the largest amplitude exceeds the second largest by 1e-4 of itself, so that float32 cannot pick another bin.
With M = 0 the gain-free cepstrum is zero whatever the input: no frame can be moved, and the case checks just that."""
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402
from make_golden_parcor import sig  # noqa: E402

ORDERS = [0, 1, 2, 24, 25, 63, 64, 100]
MODES = {"fast": {"fast": True}, "scale": {"fast": False, "mod_type": "scale"}, "clip": {"fast": False, "mod_type": "clip"}}
MARGIN, GAP = 1e-3, 1e-4
TABLE = {4: (4.5, 6.20), 5: (6.0, 7.65), 6: (7.4, 9.13), 7: (8.9, 10.6)}


def cases():
    out = []
    for M in ORDERS:   # every order in every mode at the README's options
        for mode in MODES:
            # (scale mode at M = 1: the spectrum 0.42 + e^{-jw} is so smooth that at n_fft = 256 the two largest bins are 6e-5 apart whatever
            # the input, below GAP; that order runs scale mode at n_fft = 64 and 31 instead)
            out.append({"M": M, "mode": mode, "kw": {"alpha": 0.42, "n_fft": 64} if (M, mode) == (1, "scale") else {"alpha": 0.42}})
    for mode in MODES:   # alpha = 0, the other thresholds of the table, an explicit one
        out.append({"M": 24, "mode": mode, "kw": {"alpha": 0}})
        out.append({"M": 24, "mode": mode, "kw": {"alpha": 0.42, "pade_order": 7}})
        out.append({"M": 25, "mode": mode, "kw": {"alpha": 0.42, "pade_order": 7, "strict": False}})
        out.append({"M": 24, "mode": mode, "kw": {"alpha": 0.42, "strict": False}})
        out.append({"M": 25, "mode": mode, "kw": {"alpha": 0.35, "threshold": 3.0}})
    for mode in ("scale", "clip"):   # other transform lengths: even, odd (irfft then has n_fft - 1 points), and a long one once
        for M, n_fft in ((24, 64), (63, 64), (2, 64), (1, 64), (24, 31), (25, 31), (1, 31), (0, 31)):
            out.append({"M": M, "mode": mode, "kw": {"alpha": 0.42, "n_fft": n_fft}})
    out.append({"M": 24, "mode": "clip", "kw": {"alpha": 0.42, "n_fft": 4096}})   # (clip: with bins this dense no input keeps the two largest GAP apart)
    out = [c for i, c in enumerate(out) if c not in out[:i]]
    for c in out:
        c["tag"] = "_".join([c["mode"], str(c["M"])] + [f"{k}{v}" for k, v in c["kw"].items()]).replace(".", "p")
        c["rows"] = 6 if c["M"] >= 63 else 9
    assert len({c["tag"] for c in out}) == len(out)
    return out


def threshold_of(kw):
    return kw["threshold"] if "threshold" in kw else TABLE[kw.get("pade_order", 4)][0 if kw.get("strict", True) else 1]


def amplitudes(x, mode, kw):
    """(F, K) amplitudes of the gain-free cepstrum (fast: its plain sum as one column), in float64."""
    M = x.shape[-1] - 1
    c = x.copy()
    c[:, 0] -= x @ ((-float(kw["alpha"])) ** np.arange(M + 1))
    return c.sum(-1, keepdims=True) if mode == "fast" else np.abs(np.fft.rfft(c, n=kw.get("n_fft", 256)))


def conditions(x, mode, kw, thr):
    A = amplitudes(x, mode, kw)
    a = np.maximum(A.max(-1), 1e-16)
    moved = a > thr
    ok = moved.any() and (~moved).any() and (np.abs(a - thr) >= MARGIN * thr).all()
    if mode == "clip":
        ok = ok and (np.abs(A - thr) >= MARGIN * thr).all()
    if mode == "scale":
        top = np.sort(A, -1)[:, -2:]
        ok = ok and (top[moved, 1] - top[moved, 0] >= GAP * top[moved, 1]).all()
    return bool(ok), moved


def make_input(case, seed):
    rng = np.random.default_rng(seed)
    M, rows, mode, kw = case["M"], case["rows"], case["mode"], case["kw"]
    thr = threshold_of(kw)
    x = 0.5 * rng.standard_normal((rows, M + 1)) * np.linspace(1, 0.05, M + 1)
    if M >= 1:
        a = amplitudes(x, mode, kw).max(-1) if mode != "fast" else amplitudes(x, mode, kw)[:, 0]
        want = np.where(np.arange(rows) % 3 == 0, rng.uniform(1.3, 3.0, rows), rng.uniform(0.2, 0.8, rows)) * thr
        x *= (want / a)[:, None]   # (fast: a negative sum flips the row's sign)
    return x.astype(np.float32).astype(np.float64), thr


def main():
    d = import_reference()
    F = d.functional
    cls = d.MLSADigitalFilterStabilityCheck
    out, listed = {}, []
    wrng = np.random.default_rng(20241018)
    for i, case in enumerate(cases()):
        M, mode, kw = case["M"], case["mode"], case["kw"]
        for seed in range(10000 * i, 10000 * i + 5000):
            x, thr = make_input(case, seed)
            ok, moved = conditions(x, mode, kw, thr)
            ok32, moved32 = conditions(x.astype(np.float32).astype(np.float64), mode, kw, float(np.float32(thr)))
            if M == 0 or (ok and ok32 and (moved == moved32).all()):
                break
        else:
            raise AssertionError(f"no seed satisfies the conditions of {case['tag']}")
        assert M >= 1 or not moved.any()
        w = wrng.standard_normal(x.shape).astype(np.float16).astype(np.float64)
        for name, dt in (("64", torch.float64), ("32", torch.float32)):
            xt = torch.tensor(x, dtype=dt, requires_grad=True)
            with warnings.catch_warnings(record=True) as rec:
                warnings.simplefilter("always")
                y = F.mlsacheck(xt, **MODES[mode], **kw)
            assert any("unstable" in str(r.message) for r in rec) == bool(moved.any())   # the reference detects exactly the frames this script calls moved
            (y * torch.tensor(w, dtype=dt)).sum().backward()
            assert y.shape == xt.shape
            out[f"{case['tag']}_{name}"] = np.stack([y.detach().numpy(), xt.grad.numpy()] + ([w] if name == "64" else []))
        out[f"{case['tag']}_x"] = x
        even = mode == "fast" or kw.get("n_fft", 256) % 2 == 0
        if even:   # where the transforms invert each other the reference leaves an unmoved frame within rounding of its input
            assert np.abs(out[f"{case['tag']}_64"][0] - x)[~moved].max() <= 1e-13 * max(np.abs(x).max(), 1.0)
        # clip mode at M = 0: every amplitude is exactly zero and the reference's gradient is NaN (the derivative of abs at a complex
        # zero, times threshold / 0); the output is the input.  Recorded, so that the test judges those gradients by the identity.
        nan_grad = bool(np.isnan(out[f"{case['tag']}_64"][1]).any() or np.isnan(out[f"{case['tag']}_32"][1]).any())
        assert nan_grad == (M == 0 and mode == "clip") and not np.isnan(out[f"{case['tag']}_64"][0]).any()
        listed.append({**case, "threshold": thr, "seed": seed, "moved": [bool(b) for b in moved], "ref_grad_nan": nan_grad})

    # the docstring example, mlsacheck.py:113-119
    c1 = torch.tensor([1.8963, 7.6629, 4.4804, 8.0669, -1.2768])
    out["doc_in"], out["doc_out"] = c1.numpy(), cls(cep_order=4, alpha=0.1, warn_type="ignore")(c1).numpy()
    np.savez_compressed(os.path.join(HERE, "mlsacheck.npz"), **out)

    name = "MLSADigitalFilterStabilityCheck"
    api = {"name": name, "orders": ORDERS, "cases": listed, "margin": MARGIN, "gap": GAP,
           "init": sig(cls.__init__), "forward": sig(cls.forward), "functional": sig(F.mlsacheck), "state": list(cls(3).state_dict()),
           "thresholds": {f"{p}_{s}": cls._precompute(3, 0, p, s, None, True, 256, "warn", "scale", None, None).values["threshold"]
                          for p in (4, 5, 6, 7) for s in (True, False)},
           "doc": {"printed": [1.3336, 1.7537, 1.0254, 1.8462, -0.2922], "kwargs": {"cep_order": 4, "alpha": 0.1, "warn_type": "ignore"}},
           "errors": []}
    errs = [("ctor", [-1], {}, None), ("ctor", [3], {"pade_order": 3}, None), ("ctor", [3], {"pade_order": 8}, None),
            ("ctor", [-1], {"pade_order": 8}, None), ("ctor", [3], {"pade_order": 8, "threshold": None}, None),
            ("call", [3], {}, [2, 5]), ("call", [3], {"mod_type": "clip"}, [2, 4]), ("call", [3], {"fast": False, "mod_type": "squash"}, [2, 4]),
            ("call", [3], {"mod_type": "squash"}, [2, 4]),
            ("functional", [], {"pade_order": 3}, [2, 4]), ("functional", [], {"mod_type": "clip"}, [2, 4]),
            ("functional", [], {"fast": False, "mod_type": "squash", "warn_type": "ignore"}, [2, 4])]
    for kind, args, kw, shape in errs:
        try:
            if kind == "ctor":
                cls(*args, **kw)
            elif kind == "call":
                cls(*args, **kw)(torch.zeros(shape, dtype=torch.float64))
            else:
                F.mlsacheck(torch.zeros(shape, dtype=torch.float64), *args, **kw)
            got = ["ok", ""]
        except Exception as e:   # noqa: BLE001
            got = [type(e).__name__, str(e)]
        assert got[0] != "ok", (kind, args, kw)
        api["errors"].append({"kind": kind, "args": args, "kwargs": kw, "shape": shape, "raises": got})
    # the two places where this project departs on purpose, recorded as the reference behaves
    y = F.mlsacheck(torch.zeros(2, 25, dtype=torch.float64), fast=False, n_fft=25)
    api["reference_width_at_M24_nfft25"] = int(y.size(-1))
    with open(os.path.join(HERE, "mlsacheck_api.json"), "w") as f:
        json.dump(api, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
