"""A float64 numpy restatement of PitchAdaptiveSpectralAnalysis (CheapTrick), written from the algorithm, with the gradient to the
waveform in closed form.  Per frame (b, n), f = default_f0 where f0 <= f_min = 3 sr / (L - 3), K = L / 2 + 1, rate = sr / L:

  1 window     h = round(1.5 sr / f) (ties to even), w[i] = 0.5 + 0.5 cos(pi j f / (1.5 sr)) on |j| <= h, j = i - L / 2, over its L2 norm
  2 frame      u = x[clamp(n P + j)] w + 1e-12 noise1 [|j| <= h];  s = u - w sum(u) / sum(w)
  3 power      A = |rfft(s)|^2 + eps;  R = max(A, max(A) floor)
  4 DC         D[k] = R[k] + [k rate < f] ((1 - fd) R[Bd - k] + fd R[Bd - k + 1]),  f / rate = Bd + fd
  5 smoothing  m: D reflected by b = trunc(2 f / (3 rate)) + 1 bins on both sides, seg = cumsum(m rate) from the frame's own first
               element, read linearly at k + b - 1/2 -/+ f / (3 rate); the difference over 2 f / 3
  6 noise      + |noise2| noise_eps: finfo(float64).eps in the kernels for both dtypes, finfo(dtype).eps in the reference
  7 liftering  c = irfft(log .)[:K], times sinc(f q) ((1 - 2 q1) + 2 q1 cos(2 pi f q)), q = k / sr;  hfft(.)[:K]
  8 format     0 db: 10 / ln 10 times it, 1 log-magnitude: half, 2 magnitude: exp of half, 3 power: exp

Every step but 2's clamp, 3 and the logarithm is linear in the data, so the adjoint is each step's transpose in reverse order; the
positions Bd, b and the two read offsets depend on f alone."""
import numpy as np

FORMATS = {"db": 0, "log-magnitude": 1, "magnitude": 2, "power": 3, 0: 0, 1: 1, 2: 2, 3: 3}


def frame_constants(f, sr, L):
    """what depends on f alone: (h, Bd, fd, b, Bl, fl, Bh, fh, width)"""
    rate = sr / L
    h = int(np.round(1.5 * sr / f))
    z0 = f / rate
    Bd = int(z0)
    width = f * (2 / 3)
    b = int(width / rate) + 1
    cl, ch = b - 0.5 - width / (2 * rate), b - 0.5 + width / (2 * rate)
    return h, Bd, z0 - Bd, b, int(cl), cl - int(cl), int(ch), ch - int(ch), width


def window(f, sr, L, h):
    j = np.arange(L) - L // 2
    mask = np.abs(j) <= h
    w = (0.5 + 0.5 * np.cos(np.pi * j * f / (1.5 * sr))) * mask
    return w / np.sqrt(np.sum(w * w)), mask


def reflected(K, b):
    """the index of D that position t of the mirrored spectrum holds, t in [0, K + 2 b)"""
    i = np.arange(K + 2 * b) - b
    return np.where(i < 0, -i, np.where(i > K - 1, 2 * (K - 1) - i, i))


def one_frame(xrow, n, f, P, sr, L, eps, floor, q1, fmt, n1, n2, noise_eps, gy):
    """(y:(K,), cot:(L,) or None): the frame's output and the cotangent of its L samples before the clamp"""
    K, rate, T = L // 2 + 1, sr / L, len(xrow)
    h, Bd, fd, b, Bl, fl, Bh, fh, width = frame_constants(f, sr, L)
    w, mask = window(f, sr, L, h)
    src = np.clip(n * P + np.arange(L) - L // 2, 0, T - 1)
    u = xrow[src] * w + 1e-12 * n1 * mask
    W = w.sum()
    s = u - w * (u.sum() / W)
    X = np.fft.rfft(s)
    A = X.real ** 2 + X.imag ** 2 + eps
    M = A.max()
    R = np.maximum(A, M * floor) if floor > 0 else A
    k = np.arange(K)
    dc = k * rate < f
    i0, i1 = np.clip(Bd - k, 0, K - 1), np.clip(Bd - k + 1, 0, K - 1)
    D = R + dc * ((1 - fd) * R[i0] + fd * R[i1])
    idx = reflected(K, b)
    seg = np.cumsum(D[idx] * rate)
    lo = seg[k + Bl] + (seg[k + Bl + 1] - seg[k + Bl]) * fl
    hi = seg[k + Bh] + (seg[k + Bh + 1] - seg[k + Bh]) * fh
    S = (hi - lo) / width + np.abs(n2) * noise_eps
    q = k / sr
    lifter = np.sinc(f * q) * ((1 - 2 * q1) + 2 * q1 * np.cos(2 * np.pi * f * q))
    c = np.fft.irfft(np.log(S))[:K]
    out = np.fft.hfft(c * lifter)[:K]
    y = (out * (10 / np.log(10)), out / 2, np.exp(out / 2), np.exp(out))[fmt]
    if gy is None:
        return y, None
    g = gy * (10 / np.log(10), 0.5, 0.5 * np.exp(out / 2), np.exp(out))[fmt]
    a = np.where((k == 0) | (k == K - 1), 1.0, 2.0)
    # hfft and irfft of K real values are cosine sums with the inner bins counted twice; their transposes are the same sums
    full = np.zeros(L)
    full[:K] = g
    gc = a * np.fft.fft(full).real[:K] * lifter
    full[:K] = gc
    gS = a / L * np.fft.fft(full).real[:K] / S
    # the smoothing: position u of the mirrored spectrum is inside every running sum read at or behind it
    G = np.concatenate([[0.0], np.cumsum(gS)])   # G[i + 1] = sum of gS[:i + 1]

    def upto(i):   # the sum of gS[0 .. i]
        return G[np.clip(i + 1, 0, K)]
    t = np.arange(K + 2 * b)
    gm = (-(1 - fh) * upto(t - Bh - 1) - fh * upto(t - Bh - 2) + (1 - fl) * upto(t - Bl - 1) + fl * upto(t - Bl - 2)) * (rate / width)
    gD = np.zeros(K)
    np.add.at(gD, idx, gm)
    gR = gD.copy()
    np.add.at(gR, i0[dc], (1 - fd) * gD[dc])
    np.add.at(gR, i1[dc], fd * gD[dc])
    if floor > 0:
        floored = A < M * floor
        gA = np.where(floored, 0.0, gR)
        gA[np.argmax(A)] += floor * gR[floored].sum()
    else:
        gA = gR
    gs = np.fft.irfft(2 * gA * X * np.where(a == 1, 1.0, 0.5), n=L) * L   # sum over k < K of Re(2 gA X e^{+i theta}), the inner bins once
    gu = gs - (gs * w).sum() / W
    return y, gu * w * mask


def _frames(x, f0, P, sr, L, default_f0, q1, eps, relative_floor, out_format, noise1, noise2, noise_eps, gy):
    """(y:(B, N, K), cot:(B, N, L) or None): one_frame over every frame of x:(B, T), f0:(B, N)"""
    (B, T), N, K = x.shape, f0.shape[1], L // 2 + 1
    fmt = FORMATS[out_format]
    floor = 0.0 if relative_floor is None else 10 ** (relative_floor / 10)
    f_min = 3 * sr / (L - 3)
    y = np.zeros((B, N, K))
    cot = None if gy is None else np.zeros((B, N, L))
    for bi in range(B):
        for n in range(N):
            f = default_f0 if f0[bi, n] <= f_min else f0[bi, n]
            n1 = np.zeros(L) if noise1 is None else np.asarray(noise1[bi, n], np.float64)
            n2 = np.zeros(K) if noise2 is None else np.asarray(noise2[bi, n], np.float64)
            y[bi, n], c = one_frame(x[bi], n, float(f), P, sr, L, eps, floor, q1, fmt, n1, n2, noise_eps, None if gy is None else gy[bi, n])
            if c is not None:
                cot[bi, n] = c
    return y, cot


def pitch_spec(x, f0, P, sr, L, *, default_f0=500, q1=-0.15, eps=0.0, relative_floor=None, out_format=3, noise1=None, noise2=None,
               noise_eps=float(np.finfo(np.float64).eps), gy=None):
    """x:(B, T), f0:(B, N), noise1:(B, N, L), noise2:(B, N, K) -> (y:(B, N, K), gx:(B, T) or None), float64"""
    x, f0 = np.asarray(x, np.float64), np.asarray(f0, np.float64)
    (B, T), N = x.shape, f0.shape[1]
    y, cot = _frames(x, f0, P, sr, L, default_f0, q1, eps, relative_floor, out_format, noise1, noise2, noise_eps, gy)
    gx = None if gy is None else np.zeros((B, T))
    for bi in range(B if gy is not None else 0):
        for n in range(N):
            np.add.at(gx[bi], np.clip(n * P + np.arange(L) - L // 2, 0, T - 1), cot[bi, n])
    return y, gx


def frame_cotangents(x, f0, P, sr, L, gy, *, default_f0=500, q1=-0.15, eps=0.0, relative_floor=None, out_format=3, noise1=None, noise2=None,
                     noise_eps=float(np.finfo(np.float64).eps)):
    """(B, N, L) float64: every frame's cotangent before the clamp, one_frame's second result -- what dsa_pitch_spec_vjp_frames writes
    to its scratch and pitch_spec() above adds into gx"""
    x, f0 = np.asarray(x, np.float64), np.asarray(f0, np.float64)
    return _frames(x, f0, P, sr, L, default_f0, q1, eps, relative_floor, out_format, noise1, noise2, noise_eps, np.asarray(gy, np.float64))[1]
