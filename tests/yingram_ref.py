"""Yingram restated in NumPy float64 from its formulas (not from the reference's code): the table of lags on the semitone grid, the
difference function by plain squared differences, its cumulative-mean normalisation, the linear interpolation with the integral-lag
rule, and the analytic gradient.  tests/golden/make_golden_yingram.py pins it to the reference's float64 results (1e-10 asserted, the
measured deviation recorded); tests/test_yingram_cpu.py and tests/test_gpu_yingram.py lean on it.

    d[tau]  = sum_{j < L - tau} (x[j] - x[j + tau])^2,  tau = 1 .. K - 1                     (K = lag_max)
    d'[tau] = tau d[tau] / (S_tau + 1e-7),  S_tau = sum_{k <= tau} d[k];  d'[0] = 1
    y[m]    = d'[floor_m] + w_m (d'[ceil_m] - d'[floor_m]),  w_m = lags_m - floor_m  (ceil_m = floor_m: y[m] = d'[floor_m])"""
import json
import os

import numpy as np

EPS = 1e-7
# (L, sample_rate, lag_min, lag_max, n_bin, F): the option sets of the goldens
GRID = [(32, 8000, 1, 30, 1, 3), (64, 8000, 4, 40, 3, 5), (65, 16000, 5, None, 2, 4), (256, 16000, 22, None, 4, 7),
        (400, 16000, 22, 300, 20, 3), (2048, 22050, 22, None, 20, 2)]
FUSED = dict(L=64, P=16, T=200, sample_rate=8000, lag_min=4, lag_max=40, n_bin=3)   # Frame(64, 16) on T = 200, both center values
INTEGRAL = dict(L=128, sample_rate=8800, lag_min=5, lag_max=100, n_bin=1)            # 8800 / 440 = 20: the note A4 has the lag 20
INDEX_ERRORS = [dict(frame_length=32, sample_rate=8000, lag_min=1), dict(frame_length=32, sample_rate=8000, lag_min=2, lag_max=29)]


def tables(L, sample_rate, lag_min, lag_max=None, n_bin=20):
    """(lags float64, floor int64, ceil int64, lag_max): one lag per 1 / n_bin semitone, from the first whole MIDI note at or above the
    note of lag_max up to the last whole note at or below the note of lag_min, largest lag first"""
    K = L - 1 if lag_max is None else lag_max
    note = lambda lag: 12.0 * np.log2(sample_rate / (440.0 * lag)) + 69.0   # noqa: E731
    first, last = int(np.ceil(note(K))), int(note(lag_min))
    count = int(np.ceil((last + 1 - first) / (1.0 / n_bin))) if last + 1 > first else 0   # (a range of float64 steps: the quotient as it rounds)
    midi = first + np.arange(count, dtype=np.float64) * (1.0 / n_bin)
    lags = sample_rate / (440.0 * 2.0 ** ((midi - 69.0) / 12.0))
    floor, ceil = np.floor(lags).astype(np.int64), np.ceil(lags).astype(np.int64)
    if count and ceil.max() > K - 1:
        raise ValueError(f"the largest lag {lags.max()} needs d'[{ceil.max()}], beyond lag_max - 1 = {K - 1}")
    return lags, floor, ceil, K


def difference(x, K):
    """d:(F, K) with d[:, 0] = 0"""
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[-1]
    d = np.zeros(x.shape[:-1] + (K,))
    for tau in range(1, K):
        d[..., tau] = ((x[..., :L - tau] - x[..., tau:]) ** 2).sum(-1)
    return d


def normalised(d):
    """d':(F, K) and the running sums S"""
    K = d.shape[-1]
    S = np.cumsum(d, axis=-1)
    dn = np.arange(K) * d / (S + EPS)
    dn[..., 0] = 1.0
    return dn, S


def forward(x, lags, floor, ceil, K, weight=None):
    """y:(F, M); weight: lags - floor as the module formed it (float32 modules round lags first), float64 by default"""
    w = lags - floor if weight is None else np.asarray(weight, dtype=np.float64)
    dn, _ = normalised(difference(x, K))
    return dn[..., floor] + w * (dn[..., ceil] - dn[..., floor])


def gradient(x, gy, lags, floor, ceil, K, weight=None):
    """gx:(F, L) = (dy / dx)^T gy, analytically"""
    x, gy = np.asarray(x, dtype=np.float64), np.asarray(gy, dtype=np.float64)
    w = lags - floor if weight is None else np.asarray(weight, dtype=np.float64)
    L = x.shape[-1]
    d = difference(x, K)
    _, S = normalised(d)
    gn = np.zeros_like(d)   # the cotangent of d'
    for m in range(len(lags)):
        gn[..., floor[m]] += gy[..., m] * (1.0 - w[m])
        gn[..., ceil[m]] += gy[..., m] * w[m]
    k = np.arange(K)
    q = gn * k * d / (S + EPS) ** 2
    q[..., 0] = 0.0
    gd = gn * k / (S + EPS) - np.cumsum(q[..., ::-1], axis=-1)[..., ::-1]
    gx = np.zeros_like(x)
    for tau in range(1, K):
        diff = 2.0 * gd[..., tau:tau + 1] * (x[..., :L - tau] - x[..., tau:])
        gx[..., :L - tau] += diff
        gx[..., tau:] -= diff
    return gx


def frames(x, L, P, center):
    """Frame(L, P, center) with constant padding: (T,) -> (N, L)"""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[-1]
    left = L // 2 if center else 0
    padded = np.concatenate([np.zeros(left), x, np.zeros(L - 1 - left)])
    return np.stack([padded[n * P:n * P + L] for n in range((T - 1) // P + 1)])


def unframe_adjoint(g, T, L, P, center):
    """the adjoint of frames(): (N, L) -> (T,)"""
    left = L // 2 if center else 0
    padded = np.zeros(T + L - 1)
    for n in range(g.shape[0]):
        padded[n * P:n * P + L] += g[n]
    return padded[left:left + T]


def case_id(c):
    return c["name"]


def golden_cases(golden_dir):
    """the cases of yingram_api.json with their arrays: x (float64, exact in float32), gy, y, gx, and the tables of both module dtypes"""
    api = json.load(open(os.path.join(golden_dir, "yingram_api.json")))
    z = np.load(os.path.join(golden_dir, "yingram.npz"))
    cases = []
    for c in api["cases"]:
        n = c["name"]
        arrays = {q: z[f"{n}_{q}"] for q in ("y", "gx")}
        arrays["x"] = z[f"{n}_xq"].astype(np.float64) / 4096.0
        arrays["gy"] = z[f"{n}_gq"].astype(np.float64) / 4096.0
        cases.append(dict(c, **arrays))
    return api, cases


def golden_tables(golden_dir, key):
    z = np.load(os.path.join(golden_dir, "yingram.npz"))
    return {q: z[f"tab{key}_{q}"] for q in ("lags64", "lags32", "floor", "ceil")}


def options(c):
    return dict(sample_rate=c["sample_rate"], lag_min=c["lag_min"], lag_max=c["lag_max"], n_bin=c["n_bin"])


# invalid option sets: name -> a call on the package (the reference, or this one) that raises
ERRORS = {
    "sample_rate_7999": lambda d: d.Yingram(64, sample_rate=7999),
    "lag_min_0": lambda d: d.Yingram(64, lag_min=0),
    "lag_max_L": lambda d: d.Yingram(64, lag_max=64),
    "lag_min_above_lag_max": lambda d: d.Yingram(64, lag_min=30, lag_max=29),
    "n_bin_0": lambda d: d.Yingram(64, n_bin=0),
    "wrong_frame_length": lambda d: d.Yingram(64, sample_rate=8000, lag_min=4, lag_max=40, n_bin=3)(__import__("torch").zeros(2, 63)),
}
