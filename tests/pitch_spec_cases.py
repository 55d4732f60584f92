"""The cases of PitchAdaptiveSpectralAnalysis that tests/golden/make_golden_pitch_spec.py runs through the reference and the tests run
through the restatement (tests/pitch_spec_ref.py) and the kernels.  Every input is exact in float32 -- the waveform a multiple of
1 / 4096, the noise and the cotangents multiples of 1 / 256, F0 a small dyadic rational -- and has a formula here, so the golden files
store results only."""
import functools
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
    return _margins(c["sr"], c["L"], c.get("kw", {}).get("default_f0", 500), inputs(name)[1])


def _margins(sr, L, default, f0):
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


# ------------------------------------------------------------------ below 1024 points and up to Nyquist
# The module refuses fft_length < 1024 and sample_rate < 8000; the C entries take L >= 16, so these cases call the entries themselves
# (tests/test_gpu_pitch_spec_edges.py).  The workgroup has 256 threads: L / 4 butterflies, K = L / 2 + 1 bins and L samples lie below,
# at and above it.  name -> sr, P, L; always B = 2, N = 7, T = N P and default_f0 = sr / 4, which is bin L / 4 exactly.
EDGE_CASES = {
    "L16": dict(sr=256, P=3, L=16),
    "L64": dict(sr=1024, P=5, L=64),
    "L256": dict(sr=4096, P=37, L=256),
    "L512": dict(sr=8192, P=80, L=512),
    "L1024": dict(sr=16000, P=80, L=1024),
}
EDGE_B, EDGE_N = 2, 7
# F0 per frame as a share of sr (None: 1.01 f_min, just voiced): unvoiced, a DC mask over half of the bins, a long window, and up to
# 0.49 sr, where the mask covers nearly every bin and the mirror a third of the spectrum.  The second row is 1.03 times the first;
# both are rounded to 1 / 8 Hz and capped at 0.49 sr (rounded down); no value lands within MARGIN of a tie, so none is nudged.  At L = 16, f_min = 3 sr / 13 = 0.23 sr: several frames are unvoiced
EDGE_F0 = (0.0, 0.24, 0.11, 0.45, 0.30, None, 0.49)
# each case runs twice: the plain power spectrum, and decibels with the floor and eps on
EDGE_MODES = {"power": dict(out_format=3, eps=0.0, relative_floor=None), "db_floor": dict(out_format=0, eps=1e-6, relative_floor=-60)}


def _edge_seed(name, what):
    return 7000 + 10 * list(EDGE_CASES).index(name) + what


def edge_sizes(name):
    c = EDGE_CASES[name]
    return EDGE_B, EDGE_N, EDGE_N * c["P"], c["L"], c["L"] // 2 + 1


def edge_inputs(name):
    """(x:(2, T), f0:(2, 7)) float32, exact: a sine at 0.07 sr plus noise, multiples of 1 / 4096; F0 multiples of 1 / 8 Hz"""
    c = EDGE_CASES[name]
    B, N, T, L, _ = edge_sizes(name)
    sr = c["sr"]
    rng = np.random.default_rng(_edge_seed(name, 0))
    x = np.stack([0.4 * np.sin(2 * np.pi * 0.07 * np.arange(T) + b) + 0.05 * rng.standard_normal(T) for b in range(B)])
    x = np.round(x * 4096) / 4096
    f_min = 3 * sr / (L - 3)
    row = np.asarray([1.01 * f_min if s is None else s * sr for s in EDGE_F0])
    f0 = np.stack([row * (1 + 0.03 * b) for b in range(B)])
    f0 = np.minimum(np.round(f0 * 8), np.floor(0.49 * sr * 8)) / 8
    assert np.array_equal(x, x.astype(np.float32)) and np.array_equal(f0, f0.astype(np.float32)) and f0.max() <= 0.49 * sr
    return x.astype(np.float32), f0.astype(np.float32)


def edge_noises(name):
    B, N, _, L, K = edge_sizes(name)
    return _dyadic(_edge_seed(name, 1), (B, N, L)), _dyadic(_edge_seed(name, 2), (B, N, K))


def edge_cotangent(name):
    B, N, _, _, K = edge_sizes(name)
    return _dyadic(_edge_seed(name, 3), (B, N, K))


def edge_options(name, mode):
    """(P, sr, L), the keywords of pitch_spec_ref.pitch_spec"""
    c = EDGE_CASES[name]
    return (c["P"], c["sr"], c["L"]), dict(default_f0=c["sr"] / 4, q1=-0.15, **EDGE_MODES[mode])


def edge_margins(name):
    c = EDGE_CASES[name]
    return _margins(c["sr"], c["L"], c["sr"] / 4, edge_inputs(name)[1])


def rel(a, ref):
    return float(np.abs(a - ref).max() / max(1.0, np.abs(ref).max()))


def rel_rows(a, ref):
    """the largest error of a row (the last axis) over max(1, the row's largest |ref|)"""
    return float((np.abs(a - ref).max(-1) / np.maximum(1.0, np.abs(ref).max(-1))).max())


@functools.lru_cache(maxsize=None)
def edge_reference(name, mode):
    """The restatement on the case, computed once and shared: y, gx, the frames' cotangents, and the two conditioning figures -- D_ulp, the
    largest change of y and gx when every sample moves one float64 unit in the last place (three seeded draws of the directions, as
    tests/test_gpu_pitch_spec.py::test_a_silent_waveform_with_noise_is_finite measures it), and the same measure taken row by row on the
    frames' cotangents.  Nothing here comes from a kernel."""
    import pitch_spec_ref

    x, f0 = edge_inputs(name)
    n1, n2 = edge_noises(name)
    gy = edge_cotangent(name).astype(np.float64)
    args, kw = edge_options(name, mode)
    kw = dict(kw, noise1=n1, noise2=n2)
    x = x.astype(np.float64)
    y, gx = pitch_spec_ref.pitch_spec(x, f0, *args, gy=gy, **kw)
    cot = pitch_spec_ref.frame_cotangents(x, f0, *args, gy, **kw)
    rng = np.random.default_rng(_edge_seed(name, 4))
    d = dcot = 0.0
    for _ in range(3):
        xp = np.where(rng.integers(0, 2, x.shape) == 1, np.nextafter(x, np.inf), np.nextafter(x, -np.inf))
        py, pgx = pitch_spec_ref.pitch_spec(xp, f0, *args, gy=gy, **kw)
        d = max(d, rel(py, y), rel(pgx, gx))
        dcot = max(dcot, rel_rows(pitch_spec_ref.frame_cotangents(xp, f0, *args, gy, **kw), cot))
    for a in (y, gx, cot):
        a.setflags(write=False)
    return dict(y=y, gx=gx, cot=cot, D_ulp=d, D_cot=dcot, bound=64 * max(d, 2.0 ** -53), bound_cot=64 * max(dcot, 2.0 ** -53))
