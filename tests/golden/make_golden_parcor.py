#!/usr/bin/env python3
"""Golden fixtures of lpc2par / par2lpc / lpccheck and the LAR / inverse-sine conversions, by importing the REFERENCE.
Build container only.

    python tests/golden/make_golden_parcor.py     # writes tests/golden/parcor.npz and parcor_api.json (data)

Inputs are LPC coefficients of windowed signal frames, not random PARCOR: with k_m uniform in +-0.9 the step-down recursion is so
ill-conditioned that the reference's own float32 result is useless as a yardstick (off by 8.8 at M = 24).  Three sets of FRAMES frames
each: `integ` (Hann-windowed frames of integrated noise: max|k| ~ 0.9996), `white` (white noise) and `wav` (data.wav).  Per set and
order M the input a = lpc(x, M) and its PARCOR k are stored once; per case the reference's outputs in float64 and float32, weights w
and the float64 and float32 gradients of sum(w * out).  lpc2par takes its gradient cases from `white` and `wav` only (its Jacobian grows as
|k_m| -> 1).  Every stored case passes the conditioning gate: the reference's float32 output is within GATE of its float64 output,
relative to the row maximum.  A case that does not is not stored and is listed under "gated_out" in parcor_api.json: lpc2par with
c = 2 (gamma = -1/2) at orders >= 24, where -a/2 is no stable predictor any more (the reference's float32 result is up to 0.2 off).
lpc2par with gamma = 1 must pass on every set -- lpccheck and the round trips rest on it -- and that is asserted."""
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

ORDERS = [0, 1, 2, 9, 24, 32, 33, 63]   # 32 / 33: the last order of the register kernels (DSA_PARCOR_MAX_ORDER) and the one after it
GAMMAS = [{"gamma": 1}, {"gamma": 0.9}, {"c": 2}]
MARGINS = [1e-16, 0.01]
SETS = ["integ", "white", "wav"]
FRAMES, LENGTH = 6, 400
GATE = 1e-4


def sig(f):
    return [[p.name, p.kind.name, None if p.default is inspect._empty else repr(p.default)] for p in inspect.signature(f).parameters.values()]


def frames_of(name, rng):
    if name == "wav":
        pcm = np.load(os.path.join(HERE, "datawav.npz"))["pcm"].astype(np.float64) / 32768.0
        starts = np.linspace(2000, len(pcm) - LENGTH - 1, FRAMES).astype(int)
        x = np.stack([pcm[s:s + LENGTH] for s in starts])
    elif name == "white":
        x = rng.standard_normal((FRAMES, LENGTH))
    else:
        x = np.cumsum(rng.standard_normal((FRAMES, LENGTH)), axis=-1)
    return x * np.hanning(LENGTH + 2)[1:-1]


def main():
    d = import_reference()
    F = d.functional
    rng = np.random.default_rng(20241017)
    out, gate, gated_out = {}, {}, {}

    def run(tag, fn, x64, want_grad):
        """The reference on x64 in both dtypes (+ the float64 gradient of a weighted sum), through the conditioning gate."""
        xt = torch.tensor(x64, requires_grad=True)
        y64 = fn(xt)
        y32 = fn(torch.tensor(x64, dtype=torch.float32)).double().numpy()
        e = np.abs(y32 - y64.detach().numpy()).max(-1) / np.abs(y64.detach().numpy()).max(-1)
        if e.max() > GATE:   # ill-conditioned for the reference itself: kept out, and listed
            gated_out[tag] = float(e.max())
            return
        gate[tag] = float(e.max())
        out[tag + "_f64"], out[tag + "_f32"] = y64.detach().numpy(), y32.astype(np.float32)
        if want_grad:
            w = rng.standard_normal(y64.shape).astype(np.float16)   # exact in every dtype
            (y64 * torch.tensor(w.astype(np.float64))).sum().backward()
            x32 = torch.tensor(x64, dtype=torch.float32, requires_grad=True)
            (fn(x32) * torch.tensor(w.astype(np.float32))).sum().backward()
            out[tag + "_w"], out[tag + "_grad"], out[tag + "_grad32"] = w, xt.grad.numpy(), x32.grad.numpy()

    for s in SETS:
        x = torch.tensor(frames_of(s, rng))
        for M in ORDERS:
            a = F.lpc(x, max(M, 1))[..., :M + 1].numpy()   # M = 0: the gain alone
            k = F.lpc2par(torch.tensor(a)).numpy()
            out[f"a_{s}_{M}"], out[f"k_{s}_{M}"] = a, k
            for gi, g in enumerate(GAMMAS):
                run(f"lpc2par_{s}_{M}_{gi}", lambda t: F.lpc2par(t, **g), a, s != "integ")
                run(f"par2lpc_{s}_{M}_{gi}", lambda t: F.par2lpc(t, **g), k, True)
            for mi, margin in enumerate(MARGINS):
                run(f"lpccheck_{s}_{M}_{mi}", lambda t: F.lpccheck(t, margin, "ignore"), a, True)

    assert all(v <= GATE for v in gate.values()) and not [t for t in gated_out if not (t.startswith("lpc2par") and t.endswith("_2"))], gated_out

    # the docstring examples (lpc2par.py:64-71, par2lpc.py:64-75, lpccheck.py:70-78, par2lar.py:57-64, lar2par.py:58-63, par2is.py:57-63,
    # is2par.py:57-62)
    a = d.LPC(5, 2)(d.ramp(1, 5) * 0.1)
    out["doc_a"], out["doc_k"] = a.numpy(), F.lpc2par(a).numpy()
    out["doc_a2"] = F.par2lpc(F.lpc2par(a)).numpy()
    bad = torch.tensor([1.0, -2.5, 2.8, -1.5, 0.4])
    out["doc_check_in"], out["doc_check_out"] = bad.numpy(), F.lpccheck(bad, warn_type="ignore").numpy()
    r = d.ramp(1, 4) * 0.1
    out["doc_ramp"] = r.numpy()
    for name in ("par2lar", "lar2par", "par2is", "is2par"):
        out["doc_" + name] = getattr(F, name)(r).numpy()
    # an unstable row in float64 with margin 0.01, and its gradient
    ok = F.lpc(torch.tensor(frames_of("wav", rng)[:1]), 4)[0].numpy()
    u = torch.tensor(np.stack([bad.double().numpy(), [2.0, -1.2, 1.9, -0.7, 1.3], ok]), requires_grad=True)
    y = F.lpccheck(u, 0.01, "ignore")
    w = rng.standard_normal(y.shape)
    (y * torch.tensor(w)).sum().backward()
    out["unstable_in"], out["unstable_out"], out["unstable_w"], out["unstable_grad"] = u.detach().numpy(), y.detach().numpy(), w, u.grad.numpy()
    out["unstable_k"] = F.lpc2par(u.detach()).numpy()
    np.savez_compressed(os.path.join(HERE, "parcor.npz"), **out)

    classes = {"lpc2par": "LinearPredictiveCoefficientsToParcorCoefficients", "par2lpc": "ParcorCoefficientsToLinearPredictiveCoefficients",
               "lpccheck": "LinearPredictiveCoefficientsStabilityCheck", "par2lar": "ParcorCoefficientsToLogAreaRatio",
               "lar2par": "LogAreaRatioToParcorCoefficients", "par2is": "ParcorCoefficientsToInverseSine",
               "is2par": "InverseSineToParcorCoefficients"}
    api = {"orders": ORDERS, "gammas": GAMMAS, "margins": MARGINS, "sets": SETS, "frames": FRAMES, "gate": gate, "gated_out": gated_out, "names": classes,
           "classes": {c: {"init": sig(getattr(d, c).__init__), "forward": sig(getattr(d, c).forward)} for c in classes.values()},
           "functional": {f: sig(getattr(F, f)) for f in classes},
           "state": {c: list(getattr(d, c)(3).state_dict()) for c in classes.values()}, "errors": []}
    cases = [("ctor", f, [-1], {}, None) for f in classes]
    cases += [("ctor", f, [3], kw, None) for f in ("lpc2par", "par2lpc") for kw in ({"gamma": 1.5}, {"gamma": -1.01}, {"c": 0}, {"c": -2},
                                                                                  {"gamma": 2, "c": 0})]
    cases += [("ctor", "lpccheck", [3], {"margin": m}, None) for m in (0, 1, -0.5, 1.5)]
    cases += [("ctor", "lpccheck", [-1], {"margin": 0}, None)]
    cases += [("call", f, [3], {}, [2, 5]) for f in classes]
    cases += [("functional", "lpc2par", [], {"gamma": 1.5}, [2, 4]), ("functional", "par2lpc", [], {"c": 0}, [2, 4]),
              ("functional", "lpccheck", [], {"margin": 1}, [2, 4])]
    for kind, f, args, kw, shape in cases:
        try:
            if kind == "ctor":
                getattr(d, classes[f])(*args, **kw)
            elif kind == "call":
                getattr(d, classes[f])(*args, **kw)(torch.zeros(shape, dtype=torch.float64))
            else:
                getattr(F, f)(torch.zeros(shape, dtype=torch.float64), *args, **kw)
            got = ["ok", ""]
        except Exception as e:   # noqa: BLE001
            got = [type(e).__name__, str(e)]
        api["errors"].append({"kind": kind, "module": f, "args": args, "kwargs": kw, "shape": shape, "raises": got})
    with open(os.path.join(HERE, "parcor_api.json"), "w") as f:
        json.dump(api, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
