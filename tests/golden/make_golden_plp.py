#!/usr/bin/env python3
"""Golden fixtures of PerceptualLinearPredictiveCoefficientsAnalysis (PLP) / functional.plp, by importing the REFERENCE.
Build container only.

    python tests/golden/make_golden_plp.py     # writes tests/golden/plp.npz and plp_api.json (data)

Each grid case holds a float64 power spectrum x, the reference's outputs for it in float64 and float32, weights w and the float64
gradient of sum(w * out) with respect to x.  Besides the grid: the reference's docstring example, data.wav through STFT(400, 80, 512),
the signatures, error cases and state_dict keys."""
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

# (L, C, M, n_fft, lifter, compression_factor, floor, gamma, scale, out_format, x scale)
GRID = [
    (512, 20, 12, 512, 22, 0.33, 1e-5, 0.0, "htk", "y", 1.0),
    (512, 20, 12, 512, 22, 0.33, 1e-5, 0.0, "htk", "ycE", 1.0),
    (512, 24, 12, 512, 1, 0.33, 1e-5, -0.5, "htk", "yc", 1.0),
    (512, 24, 12, 100, 3, 0.33, 1e-5, 0.0, "htk", "yE", 1.0),
    (512, 40, 24, 512, 22, 0.5, 1e-5, 0.0, "mel", "ycE", 1.0),
    (512, 26, 8, 16, 1, 0.25, 1e-3, 0.0, "bark", "y", 1e-4),
    (512, 20, 12, 100, 22, 0.33, 1e-2, -0.5, "linear", "yc", 1e-2),
    (512, 64, 62, 512, 22, 0.33, 1e-5, 0.0, "htk", "y", 1.0),
    (32, 10, 4, 16, 20, 0.33, 1e-5, 0.0, "htk", "y", 1.0),
    (32, 10, 4, 16, 1, 0.33, 1e-5, -0.5, "htk", "ycE", 1.0),
    (32, 8, 1, 16, 22, 0.33, 1e-5, 0.0, "htk", "yc", 1.0),
    (32, 12, 6, 100, 1, 0.7, 1e-5, 0.0, "mel", "yE", 1.0),
    (32, 10, 5, 512, 22, 0.33, 1e-5, -0.5, "htk", "yc", 1.0),
    (32, 9, 3, 7, 1, 0.33, 1e-5, 0.0, "htk", "ycE", 1.0),
]
FRAMES = {32: 6, 512: 3}
SR = 16000


def sig(f):
    return [[p.name, p.kind.name, None if p.default is inspect._empty else repr(p.default)] for p in inspect.signature(f).parameters.values()]


def spectrum(rng, L, F, scale):
    """Power spectra with some structure: a random smooth envelope times exponential noise."""
    K = L // 2 + 1
    k = np.arange(K)[None, :]
    env = np.exp(1.5 * np.sin(k * rng.uniform(0.02, 0.3, (F, 1)) + rng.uniform(0, 6, (F, 1))) - 2.0 * k / K)
    return scale * env * rng.exponential(1.0, (F, K))


def kwargs_of(case):
    L, C, M, n_fft, lifter, cf, floor, gamma, scale, fmt, _ = case
    return dict(fft_length=L, plp_order=M, n_channel=C, sample_rate=SR, compression_factor=cf, lifter=lifter, floor=floor,
                gamma=gamma, scale=scale, n_fft=n_fft, out_format=fmt)


def main():
    d = import_reference()
    rng = np.random.default_rng(20241016)
    out = {}
    for i, case in enumerate(GRID):
        L = case[0]
        kw = kwargs_of(case)
        x = spectrum(rng, L, FRAMES[L], case[-1])
        out[f"c{i}_x"] = x
        for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
            xt = torch.tensor(x, dtype=dt, requires_grad=True)
            y = d.PLP(**kw, dtype=dt)(xt)
            out[f"c{i}_out_{name}"] = y.detach().numpy()
            if dt == torch.float64:
                w = rng.standard_normal(y.shape)
                (y * torch.tensor(w)).sum().backward()
                out[f"c{i}_w"] = w
                out[f"c{i}_grad_f64"] = xt.grad.numpy()
    # the reference's docstring example (plp.py:141-152)
    stft = d.STFT(frame_length=10, frame_period=10, fft_length=32)
    plp = d.PLP(fft_length=32, plp_order=4, n_channel=8, sample_rate=8000)
    out["doc_x"] = d.ramp(19).numpy()
    out["doc_y"] = plp(stft(d.ramp(19))).numpy()
    # data.wav (tests/golden/datawav.npz holds the samples) through STFT(400, 80, 512) and the bench-like PLP
    pcm = np.load(os.path.join(HERE, "datawav.npz"))["pcm"]
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        xw = torch.tensor(pcm.astype(np.float64) / 32768.0, dtype=dt)
        X = d.STFT(400, 80, 512, dtype=dt)(xw)
        for fmt in ("yc", "ycE"):
            out[f"wav_{fmt}_{name}"] = d.PLP(fft_length=512, plp_order=12, n_channel=20, sample_rate=SR, lifter=22, out_format=fmt,
                                             dtype=dt)(X).numpy()
    np.savez_compressed(os.path.join(HERE, "plp.npz"), **out)

    api = {"init": sig(d.PLP.__init__), "forward": sig(d.PLP.forward), "functional": sig(d.functional.plp),
           "grid": [list(c) for c in GRID], "frames": FRAMES, "sample_rate": SR, "errors": [],
           "state_dict": {"default": list(d.PLP(fft_length=512, plp_order=12, n_channel=20, sample_rate=SR).state_dict()),
                          "learnable": list(d.PLP(fft_length=512, plp_order=12, n_channel=20, sample_rate=SR,
                                                  learnable=True).state_dict())}}
    base = dict(fft_length=512, plp_order=12, n_channel=20, sample_rate=SR)
    cases = [
        ("ctor", {"plp_order": -1}),
        ("ctor", {"n_channel": 12}),
        ("ctor", {"compression_factor": 0}),
        ("ctor", {"lifter": -1}),
        ("ctor", {"lifter": 0}),
        ("ctor", {"out_format": "cy"}),
        ("ctor", {"out_format": 4}),
        ("ctor", {"fft_length": 1}),
        ("ctor", {"sample_rate": 0}),
        ("ctor", {"f_min": 9000}),
        ("ctor", {"f_max": 9000}),
        ("ctor", {"floor": 0}),
        ("ctor", {"gamma": 1.5}),
        ("ctor", {"erb_factor": 0}),
        ("ctor", {"scale": "erb"}),
        ("ctor", {"n_fft": 13}),
        ("ctor", {"n_channel": 0, "plp_order": -1}),
        ("ctor", {"lifter": -1, "out_format": "x"}),
        ("ctor", {"out_format": "x", "floor": 0}),
        ("ctor", {"floor": 0, "n_fft": 4}),
        ("functional", {"n_fft": 13}),
        ("functional", {"plp_order": 20}),
        ("call", {}),
    ]
    for kind, kw in cases:
        try:
            if kind == "ctor":
                d.PLP(**{**base, **kw})
            elif kind == "functional":
                a = {**base, **kw}
                a.pop("fft_length")
                d.functional.plp(torch.ones(3, 257, dtype=torch.float64), **a)
            else:   # a spectrum of the wrong width
                d.PLP(**base, dtype=torch.float64)(torch.ones(3, 129, dtype=torch.float64))
            got = ["ok", ""]
        except Exception as e:   # noqa: BLE001
            got = [type(e).__name__, str(e)]
        api["errors"].append({"kind": kind, "kwargs": kw, "raises": got})
    with open(os.path.join(HERE, "plp_api.json"), "w") as f:
        json.dump(api, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
