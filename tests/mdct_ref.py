"""Shared by tests/test_mdct_cpu.py and tests/test_gpu_mdct.py: the goldens of the lapped transforms (tests/golden/mdct.npz, an index in
mdct_api.json) and the closed forms in numpy float64, written from the definitions and not from the library's tables:

  P = L/2, z = sqrt(4/P) (sqrt(2/P) for the window named "rectangular"), C[j,k] = z cos(pi/P (j + 1/2 + P/2)(k + 1/2)) (sin for "sine")
  analysis   y[n,k] = sum_j w[j] x[(n-1)P + j] C[j,k], x = 0 outside [0, T), N = (T + P - 1) // P + 1 rows
  synthesis  x[t] = s[t] sum_n w[j] sum_k y[n,k] C[j,k], j = t + P - nP, s = 1/2 for t < (N-1)P, else 1

Every function has an `absolute` form: the same sums over the magnitudes of their terms.  Its largest value is S of the float64 rule
4 L 2^-52 S -- four times the worst-case rounding of a sum of L terms (each partial sum is bounded by S; a float64 accumulation of n
terms is off by at most (n - 1) 2^-53 S to first order, the rounding of the terms and of the table entries adds 3 2^-53 S)."""
import functools
import json
import os

import numpy as np

from diffsptk_amd.utils import tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = json.load(open(os.path.join(ROOT, "tests", "golden", "mdct_api.json")))
CASES = API["cases"]
_Z = {}


def arr(name):
    """One array of the golden file (two flat arrays and the index API["arrays"]: name -> [which, offset, shape])."""
    if not _Z:
        _Z.update(np.load(os.path.join(ROOT, "tests", "golden", "mdct.npz")))
    which, off, shape = API["arrays"][name]
    return _Z[which][off:off + int(np.prod(shape, dtype=np.int64))].reshape(shape)


@functools.lru_cache(maxsize=8)
def basis(L, window, transform):
    P = L // 2
    z = (2.0 / P if window == "rectangular" else 4.0 / P) ** 0.5
    ph = np.pi / P * np.outer(np.arange(L) + 0.5 + P / 2, np.arange(P) + 0.5)
    return z * (np.cos(ph) if transform == "cosine" else np.sin(ph))


@functools.lru_cache(maxsize=8)
def window_of(L, window):
    return tables.window_table(L, window, "none", True)   # (Window(L, norm="none", symmetric=True): tested on its own elsewhere)


def overlap_scale(N, P, T_out):
    return np.where(np.arange(T_out) < (N - 1) * P, 0.5, 1.0)


def analysis(x, L, window, transform, N=None, absolute=False):
    """x:(..., T) -> (..., N, P)"""
    x = np.asarray(x, dtype=np.float64)
    P, T = L // 2, x.shape[-1]
    N = (T + P - 1) // P + 1 if N is None else N
    assert T <= N * P
    xp = np.concatenate([np.zeros((*x.shape[:-1], P)), x, np.zeros((*x.shape[:-1], N * P - T))], -1)   # (N + 1) P samples
    fr = xp[..., np.arange(N)[:, None] * P + np.arange(L)[None, :]] * window_of(L, window)
    C = basis(L, window, transform)
    return np.abs(fr) @ np.abs(C) if absolute else fr @ C


def synthesis(y, L, window, transform, T_out, scale=True, absolute=False):
    """y:(..., N, P) -> (..., T_out)"""
    y = np.asarray(y, dtype=np.float64)
    P, N = L // 2, y.shape[-2]
    assert y.shape[-1] == P and T_out <= N * P
    C, w = basis(L, window, transform), window_of(L, window)
    v = (np.abs(y) @ np.abs(C.T)) * np.abs(w) if absolute else (y @ C.T) * w
    o = np.zeros((*y.shape[:-2], (N + 1) * P))
    for n in range(N):
        o[..., n * P:n * P + L] += v[..., n, :]
    o = o[..., P:P + T_out]
    return o * overlap_scale(N, P, T_out) if scale else o


def analysis_grad(g, L, window, transform, T, absolute=False):
    """d<analysis(x), g>/dx: the synthesis of g without the division, read at T samples"""
    return synthesis(g, L, window, transform, T, scale=False, absolute=absolute)


def synthesis_grad(c, L, window, transform, N, absolute=False):
    """d<synthesis(y), c>/dy for c:(..., T_out): the analysis of c s, zero beyond T_out, with N rows"""
    c = np.asarray(c, dtype=np.float64)
    return analysis(c * overlap_scale(N, L // 2, c.shape[-1]), L, window, transform, N=N, absolute=absolute)


def synthesis_gain(L, window, transform, N=3):
    """max_t sum over the terms of x[t] of |s w C|: how far an error of the coefficients can grow in the synthesis"""
    return float(synthesis(np.ones((N, L // 2)), L, window, transform, N * (L // 2), absolute=True).max())


def rule64(L, S):
    return 4.0 * L * 2.0 ** -52 * float(S)


def amax(a):
    return float(np.abs(a).max()) if np.size(a) else 0.0
