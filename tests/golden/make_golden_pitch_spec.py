#!/usr/bin/env python3
"""Golden fixtures of PitchAdaptiveSpectralAnalysis (algorithm "cheap-trick"), by importing the REFERENCE.  Build container only (CPU;
about a minute).

    python tests/golden/make_golden_pitch_spec.py   # writes tests/golden/pitch_spec.npz, pitch_spec_b.npz and pitch_spec_api.json

The cases and the formulas of their inputs, noise and cotangents are tests/pitch_spec_cases.py (all exact in float32), so the files
hold results only: per case <name>_y and <name>_gx from the reference in float64.  The noise reaches the reference through a replaced
torch.randn_like (its two calls, in order: the frame's noise and the floor noise).

The JSON holds per case E_ref and E_gref (the reference's float32 run against its float64 run, relative to max(1, max |ref|); null where
the float32 run is not finite), restatement_deviation (tests/pitch_spec_ref.py against the reference, float64), D_ulp (the largest
relative change of the float64 results when every sample of x moves one unit in its last place, three draws), B_dep (an utterance run
alone against the same utterance in its batch: the reference's running sum starts at the batch's widest boundary) and the three tie
margins of pitch_spec_cases.margins; further the signatures, buffers, state_dict keys, the inner spec module's attributes and the
exception type and text of every invalid call of pitch_spec_cases.ERRORS.

Asserted here and again in tests/test_pitch_spec_cpu.py from the stored numbers: every margin is at least 1e-3."""
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import import_reference  # noqa: E402

import pitch_spec_cases as A  # noqa: E402
import pitch_spec_ref  # noqa: E402


class Noise:
    """Replaces torch.randn_like while a reference call runs: the given arrays, in order, in the dtype asked for."""

    def __init__(self, *arrays):
        self.arrays = list(arrays)

    def __enter__(self):
        self.saved = torch.randn_like

        def my_randn_like(t, *a, **kw):
            out = torch.as_tensor(self.arrays.pop(0)).to(t.dtype)
            assert out.shape == t.shape, (out.shape, t.shape)
            return out

        torch.randn_like = my_randn_like
        return self

    def __exit__(self, *exc):
        torch.randn_like = self.saved
        assert not self.arrays or exc[0]


def run(diffsptk, name, dtype, x, f0, n1, n2, gy):
    args, kw = A.module_args(name)
    m = diffsptk.PitchAdaptiveSpectralAnalysis(*args, **kw, dtype=dtype)
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    with Noise(n1, n2):
        y = m(xt, torch.tensor(f0, dtype=dtype))
    (y * torch.tensor(gy, dtype=dtype)).sum().backward()
    return y.detach().double().numpy(), xt.grad.double().numpy()


def rel(a, ref):
    return float(np.abs(a - ref).max() / max(1.0, np.abs(ref).max()))


def nudge(v, rng):
    v = np.asarray(v, np.float64)
    return np.where(rng.integers(0, 2, v.shape) == 1, np.nextafter(v, np.inf), np.nextafter(v, -np.inf))


def raised(f, d):
    try:
        f(d)
    except Exception as e:  # noqa: BLE001
        return [type(e).__name__, str(e)]
    return None


def signature(f):
    return [[p.name, p.kind.name, None if p.default is inspect._empty else repr(p.default)] for p in inspect.signature(f).parameters.values()]


def main():
    diffsptk = import_reference()
    out, cases = {}, []
    for name, c in A.CASES.items():
        x, f0 = A.inputs(name)
        n1, n2 = A.noises(name)
        gy = A.cotangent(name)
        sq = lambda *a: A.squeeze(name, *a)  # noqa: E731
        y64, gx64 = run(diffsptk, name, torch.float64, *sq(x, f0, n1, n2, gy))
        y32, gx32 = run(diffsptk, name, torch.float32, *sq(x, f0, n1, n2, gy))
        rec = dict(name=name, sr=c["sr"], max_y=float(np.abs(y64).max()), max_gx=float(np.abs(gx64).max()))
        rec["margin_window"], rec["margin_f_min"], rec["margin_bin"] = A.margins(name)
        assert min(rec["margin_window"], rec["margin_f_min"], rec["margin_bin"]) >= A.MARGIN, rec
        assert np.isfinite(y64).all() and np.isfinite(gx64).all(), name
        finite32 = bool(np.isfinite(y32).all() and np.isfinite(gx32).all())
        assert finite32 or name not in A.FIVE_RATES, name
        rec["E_ref"], rec["E_gref"] = (rel(y32, y64), rel(gx32, gx64)) if finite32 else (None, None)
        (P, sr, L), kw = A.module_args(name)
        fmt = kw.pop("out_format")
        ry, rgx = pitch_spec_ref.pitch_spec(x, f0, P, sr, L, out_format=fmt, noise1=n1, noise2=n2, noise_eps=float(np.finfo(np.float64).eps),
                                            gy=gy.astype(np.float64), **kw)
        rec["restatement_deviation"] = max(rel(sq(ry)[0], y64), rel(sq(rgx)[0], gx64))
        rng = np.random.default_rng(7)
        worst = 0.0
        for _ in range(3):
            y, gx = run(diffsptk, name, torch.float64, *sq(nudge(x, rng), f0, n1, n2, gy))
            worst = max(worst, rel(y, y64), rel(gx, gx64))
        rec["D_ulp"] = worst
        if x.shape[0] > 1:
            worst = 0.0
            for b in range(x.shape[0]):
                y, gx = run(diffsptk, name, torch.float64, x[b:b + 1], f0[b:b + 1], n1[b:b + 1], n2[b:b + 1], gy[b:b + 1])
                worst = max(worst, rel(y[0], y64[b]), rel(gx[0], gx64[b]))
            rec["B_dep"] = worst
        else:
            rec["B_dep"] = 0.0
        out[name] = {f"{name}_y": y64, f"{name}_gx": gx64}
        cases.append(rec)
        print(rec, flush=True)
    cls = diffsptk.PitchAdaptiveSpectralAnalysis
    buffers, spec = {}, {}
    for key, dtype in (("float32", None), ("float64", torch.float64)):
        m = cls(80, 16000, 1024, dtype=dtype)
        buffers[key] = {k: [str(v.dtype), list(v.shape)] for k, v in m.named_buffers()}
    e = cls(80, 16000, 1024, eps=1e-6, relative_floor=-60).extractor
    attributes = {k: repr(getattr(e, k)) for k in ("frame_period", "sample_rate", "fft_length", "f_min", "q1", "default_f0")}
    api = {
        "cases": cases,
        "signatures": {"__init__": signature(cls.__init__), "forward": signature(cls.forward),
                       "extractor.__init__": signature(type(e).__init__), "extractor.forward": signature(type(e).forward)},
        "buffers": buffers,
        "attributes": attributes,
        "spec_class": type(e.spec).__name__,
        "state_dict": sorted(cls(80, 16000, 1024).state_dict()),
        "in_root": hasattr(diffsptk, "PitchAdaptiveSpectralAnalysis"),
        "in_functional": any("pitch_spec" in n for n in dir(diffsptk.functional)),
        "errors": {n: raised(f, diffsptk) for n, f in A.ERRORS.items()},
    }
    for file, names in A.FILES.items():
        blob = {}
        for n in names:
            blob.update(out[n])
        np.savez_compressed(os.path.join(HERE, file), **blob)
        size = os.path.getsize(os.path.join(HERE, file))
        print(file, size)
        assert size < 1 << 20, (file, size)
    assert sorted(n for names in A.FILES.values() for n in names) == sorted(A.CASES)
    with open(os.path.join(HERE, "pitch_spec_api.json"), "w") as f:
        json.dump(api, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
