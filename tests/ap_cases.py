"""The cases of Aperiodicity that tests/golden/make_golden_ap.py runs through the reference and the tests run through the restatement and the
kernels.  Every input is exact in float32: the waveform is a multiple of 1 / 4096, F0 a small dyadic rational."""
import json
import os

import numpy as np

FORMATS = {"a": 0, "p": 1, "a/p": 2, "p/a": 3}
# F0 per frame: values <= 32 (they read as 150), a jump, one very high value; no tmp_fs / f0 near a half-integer
F0_ROW = (203.0, 0.0, 20.0, 211.0, 223.0, 397.0, 101.0, 149.0, 32.0, 997.0, 127.0, 251.0)

# name -> sr, P, L, and optionally fmt, B, N, T, scale (of F0 per row), silent (samples set to zero), noise, kw
CASES = {
    "band8k": dict(sr=8000, P=40, L=None),
    "ties8k": dict(sr=8000, P=25, L=16),     # odd P: n P tmp_fs / sr + 1.5 is an exact integer in the deep bands
    "bins16k": dict(sr=16000, P=80, L=64),
    "fmt_a": dict(sr=16000, P=80, L=512, fmt="a"),
    "fmt_p": dict(sr=16000, P=80, L=512, fmt="p"),
    "fmt_ap": dict(sr=16000, P=80, L=512, fmt="a/p"),
    "fmt_pa": dict(sr=16000, P=80, L=512, fmt="p/a"),
    "wide48k": dict(sr=48000, P=240, L=2048),
    "batched": dict(sr=16000, P=80, L=64, B=3, N=15, scale=(1.0, 1.5, 0.75)),   # N is f0's own: three frames past the waveform
    "shortest": dict(sr=16000, P=7, L=64, T=81),   # 81 samples: the pyramid's minimum at 16 kHz
    "silent": dict(sr=16000, P=80, L=64, silent=(0, 760)),
    "options": dict(sr=16000, P=80, L=64, kw=dict(window_length_ms=20, eps=1e-4)),
}
SILENT = "silent"
GROUPS = sorted({c["sr"] for c in CASES.values()})


def inputs(name):
    """(x:(B, T) float32, f0:(B, N) float32, gy seed) of a case; B = 1 unless the case says otherwise"""
    c = CASES[name]
    B, N = c.get("B", 1), c.get("N", 12)
    T = c.get("T", 12 * c["P"])
    rng = np.random.default_rng(sorted(CASES).index(name) + 1)
    t = np.arange(T) / c["sr"]
    scale = c.get("scale", (1.0,) * B)
    x = np.stack([0.4 * np.sin(2 * np.pi * 203 * scale[b] * t) + 0.2 * np.sin(2 * np.pi * 406 * scale[b] * t + 1.0) +
                  c.get("noise", 0.05) * rng.standard_normal(T) for b in range(B)])
    x = np.round(x * 4096) / 4096
    if "silent" in c:
        x[:, c["silent"][0]:c["silent"][1]] = 0
    f0 = np.stack([np.resize(np.asarray(F0_ROW), N) * scale[b] for b in range(B)])
    assert np.array_equal(x, x.astype(np.float32)) and np.array_equal(f0, f0.astype(np.float32))
    return x.astype(np.float32), f0.astype(np.float32)


def cotangent(name, shape):
    """the stored cotangent's formula: multiples of 1 / 256, exact in float32"""
    rng = np.random.default_rng(1000 + sorted(CASES).index(name))
    return (np.round(rng.standard_normal(shape) * 256) / 256).astype(np.float32)


def module_args(name):
    c = CASES[name]
    return (c["P"], c["sr"], c["L"]), dict(out_format=c.get("fmt", "a"), **c.get("kw", {}))


def half_integer_margin(name):
    """the smallest distance of pitch + 0.5 and pitch / 2 + 0.5 from an integer over the case's bands and frames, in float64"""
    from diffsptk_amd.ops.ap import ap_bands

    c = CASES[name]
    _, f0 = inputs(name)
    f = np.where(f0 <= 32, 150.0, f0.astype(np.float64))
    _, cutoff, _ = ap_bands(c["sr"])
    worst = 1.0
    for cut in cutoff:
        for v in (2 * cut / f + 0.5, 2 * cut / f * 0.5 + 0.5):
            worst = min(worst, float(np.abs(v - np.round(v)).min()))
    return worst


# A clean float64 sinusoid with a regulariser far below the rounding of R = H' W H: the 6 x 6 systems are singular to working precision,
# the first trials fail on a pivot that is rounding noise, and a later m = 10, 100, ... factors them.  lower_bound 0 keeps the values.
ESCALATING = dict(sr=16000, P=80, N=12, eps=1e-22, lower=0.0)


def escalating_inputs():
    """(x:(1, T), f0:(1, N)) float64"""
    c = ESCALATING
    t = np.arange(c["N"] * c["P"]) / c["sr"]
    return (0.5 * np.sin(2 * np.pi * 220 * t))[None], np.full((1, c["N"]), 220.0)


def escalating_sensitivity(ap_ref, x, f0, gy, trials, draws=3):
    """(D_y, D_gx): the largest change of the restatement's results, relative to max(1, max |ref|), when every sample of x moves one unit
    in its last place, the fits held to the given trials.  Over the fits whose factor succeeds there before and after the move; the
    cotangent of the others is set to zero (with fft_length None every output position belongs to one fit), so they add nothing to gx"""
    c = ESCALATING
    kw = dict(lower=c["lower"], eps=c["eps"], trials=trials)
    d0 = {}
    ap_ref.aperiodicity(x, f0, c["P"], c["sr"], None, detail=d0, **kw)
    ok0 = fit_mask(d0["fits"])
    rng = np.random.default_rng(21)
    worst_y = worst_g = 0.0
    for _ in range(draws):
        xp = np.where(rng.integers(0, 2, x.shape) == 1, np.nextafter(x, np.inf), np.nextafter(x, -np.inf))
        d = {}
        ap_ref.aperiodicity(xp, f0, c["P"], c["sr"], None, detail=d, **kw)
        both = ok0 & fit_mask(d["fits"])
        y0, g0 = ap_ref.aperiodicity(x, f0, c["P"], c["sr"], None, gy=gy * both, **kw)
        y, g = ap_ref.aperiodicity(xp, f0, c["P"], c["sr"], None, gy=gy * both, **kw)
        worst_y = max(worst_y, float(np.abs(y - y0)[both].max() / max(1.0, np.abs(y0).max())))
        worst_g = max(worst_g, float(np.abs(g - g0).max() / max(1.0, np.abs(g0).max())))
    return worst_y, worst_g


def fit_mask(fits):
    """(B, N, n_band + 1) bool: which output positions come from a fit that factored (position d: band n_band - d; 0: the lowest again)"""
    ok = [f.ok for f in fits]
    return np.stack([ok[-1]] + ok[::-1], -1)


def _zeros(*shape):
    import torch

    return torch.zeros(*shape)


ERRORS = {
    "frame_period": lambda d: d.Aperiodicity(0, 16000),
    "sample_rate": lambda d: d.Aperiodicity(80, 7999),
    "fft_length": lambda d: d.Aperiodicity(80, 16000, 15),
    "bounds": lambda d: d.Aperiodicity(80, 16000, 64, lower_bound=0.5, upper_bound=0.5),
    "algorithm": lambda d: d.Aperiodicity(80, 16000, 64, algorithm="straight"),
    "out_format": lambda d: d.Aperiodicity(80, 16000, 64, out_format="x"),
    "window_length_ms": lambda d: d.Aperiodicity(80, 16000, 64, window_length_ms=0),
    "eps": lambda d: d.Aperiodicity(80, 16000, 64, eps=0),
    "x_ndim": lambda d: d.Aperiodicity(80, 16000, 64)(_zeros(1, 2, 960), _zeros(2, 12)),
    "f0_ndim": lambda d: d.Aperiodicity(80, 16000, 64)(_zeros(2, 960), _zeros(1, 2, 12)),
}


def load(golden_dir):
    with open(os.path.join(golden_dir, "ap_api.json")) as f:
        api = json.load(f)
    return api, np.load(os.path.join(golden_dir, "ap.npz"))
