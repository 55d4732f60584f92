"""Shared by tests/test_paramgen_cpu.py and tests/test_gpu_paramgen.py: the goldens of delta / mlpg / mcpf (tests/golden/paramgen.npz, an
index in paramgen_api.json) and the closed forms in numpy float64, written from the definitions and not from the library's tables:

  delta   y[t,h,d] = sum_j window[h,j] x[clamp(t + j - N, 0, T - 1), d]; its adjoint is a scatter-add here (the kernels gather)
  mlpg    W[(t,h), s] = window[h, s - t + N], kept where t < N ? th[h] <= t : (t > T - N - 1 ? th[h] < T - t : True); c = (W^T W)^-1 W^T u
          with W dense here (the test shapes are small), and the band of W^T W for the library's host tables to be held against
  mcpf    out = w * mc, out[0] += log(e1 / e2) / 2, e = sum_k u_k exp(2 s_k), s = R mc (R w mc for e2), R = cos(2 pi k m / n) A^T with A
          the freqt matrix of -alpha (diffsptk_amd.utils.tables.freqt_matrix, tested on its own elsewhere); u = 1, 2, .., 2, 1"""
import json
import os

import numpy as np

from diffsptk_amd.utils import tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = json.load(open(os.path.join(ROOT, "tests", "golden", "paramgen_api.json")))
DELTA_CASES, MLPG_CASES, MCPF_CASES = API["delta_cases"], API["mlpg_cases"], API["mcpf_cases"]
SEEDS = API["seeds"]
_Z = {}


def arr(name):
    """One array of the golden file (two flat arrays and the index API["arrays"]: name -> [which, offset, shape])."""
    if not _Z:
        _Z.update(np.load(os.path.join(ROOT, "tests", "golden", "paramgen.npz")))
    which, off, shape = API["arrays"][name]
    return _Z[which][off:off + int(np.prod(shape, dtype=np.int64))].reshape(shape)


def amax(a):
    return float(np.abs(a).max()) if np.size(a) else 0.0


def window_of(seed, static_out=True):
    """(H, L), L odd: delta.py:105-178 restated"""
    if isinstance(seed[0], (tuple, list)):
        rows = ([[1.0]] if static_out else []) + [list(map(float, c)) for c in seed]
        L = max(map(len, rows)) | 1
        return np.array([[0.0] * ((L - len(c)) // 2) + c + [0.0] * (L - len(c) - (L - len(c)) // 2) for c in rows])
    L = 2 * max(seed) + 1
    w = np.zeros((int(static_out) + len(seed), L))
    if static_out:
        w[0, L // 2] = 1
    j = np.arange(L) - L // 2
    n = seed[0]
    w[int(static_out)] = np.where(abs(j) <= n, j / (n * (n + 1) * (2 * n + 1) / 3), 0)
    if len(seed) > 1:
        n = seed[1]
        a0 = 2 * n + 1
        a1 = a0 * n * (n + 1) / 3
        a2 = a1 * (3 * n * n + 3 * n - 1) / 5
        w[int(static_out) + 1] = np.where(abs(j) <= n, (a0 * j * j - a1) / (2 * (a2 * a0 - a1 * a1)), 0)
    return w


def th_of(seed):
    return np.array([0] + ([len(c) // 2 for c in seed] if isinstance(seed[0], (tuple, list)) else list(seed)))


def delta(x, window):
    """x:(..., T, D) -> (..., T, H D)"""
    x = np.asarray(x, dtype=np.float64)
    T, D = x.shape[-2:]
    H, L = window.shape
    N = (L - 1) // 2
    idx = np.clip(np.arange(T)[:, None] + np.arange(L)[None, :] - N, 0, T - 1)   # (T, L)
    y = np.einsum("hj,...tjd->...thd", window, x[..., idx, :])
    return y.reshape(*x.shape[:-2], T, H * D)


def delta_adjoint(g, window):
    """g:(..., T, H D) -> (..., T, D)"""
    g = np.asarray(g, dtype=np.float64)
    H, L = window.shape
    T, D = g.shape[-2], g.shape[-1] // H
    N = (L - 1) // 2
    g = g.reshape(*g.shape[:-2], T, H, D)
    out = np.zeros((*g.shape[:-3], T, D))
    for t in range(T):
        for j in range(L):
            out[..., min(max(t + j - N, 0), T - 1), :] += np.einsum("h,...hd->...d", window[:, j], g[..., t, :, :])
    return out


def mlpg_matrix(T, window, th):
    """W:(T H, T) from the edge rules of mlpg.py:146-156"""
    H, L = window.shape
    N = (L - 1) // 2
    assert T >= 2 * N
    W = np.zeros((T, H, T))
    for t in range(T):
        keep = (th <= t) if t < N else ((th < T - t) if t > T - N - 1 else np.ones(H, bool))
        for j in range(L):
            s = t + j - N
            if 0 <= s < T:
                W[t, :, s] = window[:, j] * keep
    return W.reshape(T * H, T)


def mlpg_band(T, window, th):
    """(T, 2N + 1): band[s, i] = (W^T W)[s, s - 2N + i], 0 left of column 0; asserts that nothing lies outside the band"""
    W = mlpg_matrix(T, window, th)
    A = W.T @ W
    K = window.shape[1] - 1
    band = np.zeros((T, K + 1))
    for s in range(T):
        for i in range(K + 1):
            if s - K + i >= 0:
                band[s, i] = A[s, s - K + i]
    assert np.all(np.triu(A, K + 1) == 0) and np.allclose(A, A.T, atol=0)
    return band


def mlpg(u, window, th):
    """u:(..., T, D H) h-major -> (..., T, D)"""
    u = np.asarray(u, dtype=np.float64)
    H = window.shape[0]
    T, D = u.shape[-2], u.shape[-1] // H
    W = mlpg_matrix(T, window, th)
    r = np.einsum("Ts,...Td->...sd", W, u.reshape(*u.shape[:-2], T * H, D))
    return np.moveaxis(np.linalg.solve(W.T @ W, np.moveaxis(r, -2, 0).reshape(T, -1)).reshape(T, *r.shape[:-2], D), 0, -2)


def mlpg_adjoint(g, window, th):
    """g:(..., T, D) -> (..., T, D H)"""
    g = np.asarray(g, dtype=np.float64)
    H = window.shape[0]
    T, D = g.shape[-2:]
    W = mlpg_matrix(T, window, th)
    v = np.linalg.solve(W.T @ W, np.moveaxis(g, -2, 0).reshape(T, -1))
    return np.moveaxis((W @ v).reshape(T, H, *g.shape[:-2], D), (0, 1), (-3, -2)).reshape(*g.shape[:-2], T, H * D)


def _mcpf_parts(mc, alpha, beta, onset, ir_length):
    mc = np.asarray(mc, dtype=np.float64)
    M1 = mc.shape[-1]
    n = ir_length
    bins = n // 2 + 1
    A = tables.freqt_matrix(M1 - 1, n - 1, -alpha)   # (M1, n): the de-warped cepstrum is mc @ A
    R = np.cos(2 * np.pi / n * np.outer(np.arange(bins), np.arange(n))) @ A.T   # (bins, M1)
    w = np.where(np.arange(M1) < onset, 1.0, 1.0 + beta)
    uk = np.full(bins, 2.0)
    uk[0] = uk[-1] = 1.0
    q1 = uk * np.exp(2 * mc @ R.T)
    q2 = uk * np.exp(2 * (mc * w) @ R.T)
    return mc, R, w, q1, q2


def mcpf(mc, alpha, beta, onset, ir_length):
    mc, R, w, q1, q2 = _mcpf_parts(mc, alpha, beta, onset, ir_length)
    out = mc * w
    out[..., 0] += 0.5 * np.log(q1.sum(-1) / q2.sum(-1))
    return out


def mcpf_grad(mc, g, alpha, beta, onset, ir_length):
    """d<mcpf(mc), g>/dmc"""
    mc, R, w, q1, q2 = _mcpf_parts(mc, alpha, beta, onset, ir_length)
    g = np.asarray(g, dtype=np.float64)
    p1, p2 = q1 / q1.sum(-1, keepdims=True), q2 / q2.sum(-1, keepdims=True)
    return w * g + g[..., :1] * (p1 @ R - w * (p2 @ R))
