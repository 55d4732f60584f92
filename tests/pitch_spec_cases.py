"""The cases of PitchAdaptiveSpectralAnalysis that tests/golden/make_golden_pitch_spec.py runs through the reference and the tests run
through the restatement (tests/pitch_spec_ref.py) and the kernels.  Every input is exact in float32 -- the waveform a multiple of
1 / 4096, the noise and the cotangents multiples of 1 / 256, F0 a small dyadic rational -- and has a formula here, so the golden files
store results only."""
import json
import os

import numpy as np

FORMATS = {"db": 0, "log-magnitude": 1, "magnitude": 2, "power": 3, 0: 0, 1: 1, 2: 2, 3: 3}
# F0 per frame: unvoiced, below f_min, voiced low and high, jumps; the second row of a batch is 1.5 times this one
F0_ROW = (203.0, 0.0, 47.5, 211.0, 223.0, 397.0, 101.0, 149.0, 55.0, 797.0, 31.0, 1013.0)
MARGIN = 1e-3   # what every tie keeps clear of (Hz, or window samples)

# name -> sr, P, L, and optionally B, N, fmt, kw, unbatched, nonoise
CASES = {
    "k16": dict(sr=16000, P=80, L=1024),
    "odd8k": dict(sr=8000, P=37, L=1024),
    "wide48k": dict(sr=48000, P=240, L=2048),
    "short": dict(sr=16000, P=80, L=1024, N=5),     # T = 400 < L / 2: every frame is mostly padding
    "dense": dict(sr=16000, P=7, L=1024),
    "ceiling": dict(sr=96000, P=480, L=4096, B=1, N=3),
    "options": dict(sr=16000, P=80, L=1024, kw=dict(eps=1e-6, relative_floor=-60, q1=-0.1, default_f0=300)),
    "fmt_db": dict(sr=16000, P=80, L=1024, fmt="db"),
    "fmt_logmag": dict(sr=16000, P=80, L=1024, fmt=1),
    "fmt_mag": dict(sr=16000, P=80, L=1024, fmt="magnitude"),
    "fmt_power": dict(sr=16000, P=80, L=1024, fmt=3),
    "unbatched": dict(sr=16000, P=80, L=1024, B=1, unbatched=True),
    "nonoise": dict(sr=16000, P=80, L=1024, nonoise=True),
}
FILES = {"pitch_spec.npz": ("k16", "odd8k", "wide48k", "short", "dense", "ceiling"),
         "pitch_spec_b.npz": ("options", "fmt_db", "fmt_logmag", "fmt_mag", "fmt_power", "unbatched", "nonoise")}
FIVE_RATES = ("k16", "odd8k", "wide48k", "short", "dense")   # the reference is finite on these in both dtypes


def _seed(name, what):
    return 1000 * what + sorted(CASES).index(name) + 1


def sizes(name):
    c = CASES[name]
    B, N = c.get("B", 2), c.get("N", 12)
    return B, N, N * c["P"], c["L"], c["L"] // 2 + 1


def inputs(name):
    """(x:(B, T), f0:(B, N)) float32; T = N P, so that f0 has the (T - 1) // P + 1 frames of the waveform"""
    c = CASES[name]
    B, N, T, _, _ = sizes(name)
    rng = np.random.default_rng(_seed(name, 0))
    t = np.arange(T) / c["sr"]
    x = np.stack([0.4 * np.sin(2 * np.pi * 203 * (1 + 0.5 * b) * t) + 0.2 * np.sin(2 * np.pi * 406 * (1 + 0.5 * b) * t + 1.0) +
                  0.05 * rng.standard_normal(T) for b in range(B)])
    x = np.round(x * 4096) / 4096
    f0 = np.stack([np.resize(np.asarray(F0_ROW), N) * (1 + 0.5 * b) for b in range(B)])
    assert np.array_equal(x, x.astype(np.float32)) and np.array_equal(f0, f0.astype(np.float32))
    return x.astype(np.float32), f0.astype(np.float32)


def _dyadic(seed, shape):
    return (np.round(np.random.default_rng(seed).standard_normal(shape) * 256) / 256).astype(np.float32)


def noises(name):
    """(noise1:(B, N, L), noise2:(B, N, K)) float32: what the two randn_like calls of the reference return, in their order"""
    B, N, _, L, K = sizes(name)
    n1, n2 = _dyadic(_seed(name, 1), (B, N, L)), _dyadic(_seed(name, 2), (B, N, K))
    return (np.zeros_like(n1), np.zeros_like(n2)) if CASES[name].get("nonoise") else (n1, n2)


def cotangent(name):
    B, N, _, _, K = sizes(name)
    return _dyadic(_seed(name, 3), (B, N, K))


def module_args(name):
    c = CASES[name]
    return (c["P"], c["sr"], c["L"]), dict(out_format=c.get("fmt", "power"), **c.get("kw", {}))


def squeeze(name, *arrays):
    """the arrays as the module gets them: without the batch axis in the unbatched case"""
    return tuple(a[0] for a in arrays) if CASES[name].get("unbatched") else arrays


def margins(name):
    """(window, f_min, bin): the smallest distance of 1.5 sr / f from a half-integer (where round() ties), of f0 from f_min (Hz), and of f
    from a multiple of sr / L (Hz; where the DC mask k sr / L < f flips) -- the last one without the default F0 when that is an exact
    multiple: the comparison is then exact in every precision and `<` is false"""
    c = CASES[name]
    sr, L = c["sr"], c["L"]
    default = c.get("kw", {}).get("default_f0", 500)
    _, f0 = inputs(name)
    f0 = f0.astype(np.float64)
    f_min = 3 * sr / (L - 3)
    f = np.where(f0 <= f_min, float(default), f0)
    v = 1.5 * sr / f
    rate = sr / L
    r = f / rate
    off = np.abs(r - np.round(r)) * rate
    exact = (f == default) & (default / rate == np.round(default / rate))
    return float(np.abs(v - np.floor(v) - 0.5).min()), float(np.abs(f0 - f_min).min()), float(off[~exact].min())


def _zeros(*shape):
    import torch

    return torch.zeros(*shape)


ERRORS = {
    "frame_period": lambda d: d.PitchAdaptiveSpectralAnalysis(0, 16000, 1024),
    "sample_rate": lambda d: d.PitchAdaptiveSpectralAnalysis(80, 7999, 1024),
    "fft_length": lambda d: d.PitchAdaptiveSpectralAnalysis(80, 16000, 512),
    "algorithm": lambda d: d.PitchAdaptiveSpectralAnalysis(80, 16000, 1024, algorithm="x"),
    "out_format": lambda d: d.PitchAdaptiveSpectralAnalysis(80, 16000, 1024, out_format="x"),
    "default_f0": lambda d: d.PitchAdaptiveSpectralAnalysis(80, 16000, 1024, default_f0=40),
    "eps": lambda d: d.PitchAdaptiveSpectralAnalysis(80, 16000, 1024, eps=-1),
    "relative_floor": lambda d: d.PitchAdaptiveSpectralAnalysis(80, 16000, 1024, relative_floor=1),
    "unknown_keyword": lambda d: d.PitchAdaptiveSpectralAnalysis(80, 16000, 1024, window_length_ms=30),
}


def load(golden_dir):
    with open(os.path.join(golden_dir, "pitch_spec_api.json")) as f:
        api = json.load(f)
    z = {}
    for file in FILES:
        z.update(np.load(os.path.join(golden_dir, file)))
    return api, z
