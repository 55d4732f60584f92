"""A float64 numpy restatement of Aperiodicity (algorithm "tandem"), forward and gradient to x, written from the formulas of
include/diffsptk_amd.h, section a25 -- not from the kernel: whole-array gathers, einsum, np.add.at.  The integers t0, index_bias and
curr_pos are formed in the dtype asked for, everything else in float64; the regulariser escalates per fit."""
import numpy as np

# the restatement's own copy of the QMF pair (first half and centre tap of each symmetric filter) and of the band rule
_HIGH = (4.1447996898231424e-4, 7.8125051417292477e-4, -1.0917236836275842e-3, -1.9867925675967589e-3, 2.0903896961562292e-3,
         4.0940570272849346e-3, -3.4025808529816698e-3, -7.4961541272056016e-3, 4.9722633399330637e-3, 1.2738791249119802e-2,
         -6.6960326895749113e-3, -2.0694051570247052e-2, 8.4324365650413451e-3, 3.3074383758700532e-2, -1.0018936738799522e-2,
         -5.4231361405808247e-2, 1.1293988915051487e-2, 1.0020081367388213e-1, -1.2120546202484579e-2, -3.1630021039095702e-1,
         5.1240682580627639e-1)
_LOW = (-6.5488170077483048e-4, 7.561994958159384e-5, 2.0408456937895227e-3, -7.4680535322030437e-4, -4.3502235688264931e-3,
        2.5966428382642732e-3, 7.6396022827566962e-3, -6.4904118901497852e-3, -1.1765804538954506e-2, 1.3649908479276255e-2,
        1.636866479016021e-2, -2.6075976030529347e-2, -2.0910294856659444e-2, 4.8260725032316647e-2, 2.4767846611048111e-2,
        -9.6178467583360641e-2, -2.7359756709866623e-2, 3.1488052161630042e-1, 5.2827343594055032e-1)
HH = np.asarray(_HIGH + _HIGH[-2::-1])
HL = np.asarray(_LOW + _LOW[-2::-1])
TRIALS = 9


def ap_bands(sr, window_length_ms=30):
    """(n_band, cutoffs, segments): floor(log2(sr / 600)) bands, cutoff sr / 4, sr / 8, ... with the last one twice"""
    n_band = int(np.floor(np.log2(sr / 600)))
    cutoff = [sr / 2 ** min(i + 2, n_band) for i in range(n_band)]
    return n_band, cutoff, [int(c * window_length_ms / 500 + 1.5) for c in cutoff]


def qmf(x):
    """(B, T) -> high-pass, low-pass (B, ceil(T / 2))"""
    xp = np.pad(x, ((0, 0), (20, 20)), mode="reflect")
    hp = np.stack([np.convolve(r, HH, "valid")[::2] for r in xp])
    lp = np.stack([np.convolve(r[2:-2], HL, "valid")[::2] for r in xp])
    return hp, lp


def qmf_vjp(ghp, glp, T):
    B = ghp.shape[0]
    gxp = np.zeros((B, T + 40))
    for b in range(B):
        up = np.zeros(T)
        up[::2] = ghp[b]
        gxp[b] += np.convolve(up, HH, "full")
        up[::2] = glp[b]
        gxp[b, 2:-2] += np.convolve(up, HL, "full")
    gx = gxp[:, 20:20 + T].copy()
    gx[:, 1:21] += gxp[:, :20][:, ::-1]
    gx[:, T - 21:T - 1] += gxp[:, T + 20:][:, ::-1]
    return gx


def pyramid(x, n_band):
    bands, low = [], x
    for _ in range(n_band - 1):
        hp, low = qmf(low)
        bands.append(hp)
    bands.append(low)
    return bands


def decisions(f0, P, sr, fs, dtype):
    """t0, index_bias:(B, N) and curr_pos:(N) of one band, in `dtype` with the reference's operations in its order"""
    dt = np.dtype(dtype).type
    f = np.asarray(f0).astype(dtype)
    f = np.where(f <= 32, dt(150), f)
    pitch = dt(fs) / f
    t0 = (pitch + dt(0.5)).astype(np.int32)
    bias = (pitch * dt(0.5) + dt(0.5)).astype(np.int32)
    time = np.arange(f.shape[-1], dtype=dtype) * dt(P / sr)
    cpos = (time * dt(fs) + dt(1.5)).astype(np.int32)
    assert pitch.dtype == time.dtype == np.dtype(dtype)
    return t0.astype(np.int64), bias.astype(np.int64), cpos.astype(np.int64)


def _cholesky(R, lam):
    L = np.zeros_like(R)
    ok = np.ones(R.shape[:-2], bool)
    with np.errstate(all="ignore"):
        for r in range(6):
            for c in range(r + 1):
                s = R[..., r, c] - np.einsum("...k,...k->...", L[..., r, :c], L[..., c, :c])
                if r == c:
                    s = s + lam
                    ok &= (s > 0) & np.isfinite(s)
                    L[..., r, r] = np.sqrt(np.where(s > 0, s, 1.0))
                else:
                    L[..., r, c] = s / L[..., c, c]
    return L, ok


def _solve(L, rhs):
    t = np.zeros_like(rhs)
    for r in range(6):
        t[..., r] = (rhs[..., r] - np.einsum("...k,...k->...", L[..., r, :r], t[..., :r])) / L[..., r, r]
    out = np.zeros_like(rhs)
    for r in range(5, -1, -1):
        out[..., r] = (t[..., r] - np.einsum("...k,...k->...", L[..., r + 1:, r], out[..., r + 1:])) / L[..., r, r]
    return out


class Fit:
    """One band: the gathers, the regularised solve with its per-fit escalation, the ratio of stds; .vjp(gA) -> the band's gradient."""

    def __init__(self, xb, f0, P, sr, fs, J, eps, upper, dtype, trials=None):
        B, Tb = xb.shape
        t0, bias, cpos = decisions(f0, P, sr, fs, dtype)
        self.t0, self.bias, self.cpos = t0, bias, cpos
        origin = cpos[None, :] - bias
        p = np.arange(J + 2)
        rows = np.arange(B)[:, None, None]
        self.idx = [np.clip((s - 1)[..., None] + p, 0, Tb - 1) for s in (origin - t0, origin + t0, origin)]
        ra, rb, rg = (xb[rows, i] for i in self.idx)
        self.H = H = np.stack([ra[..., 0:J], ra[..., 1:J + 1], ra[..., 2:J + 2], rb[..., 0:J], rb[..., 1:J + 1], rb[..., 2:J + 2]], -1)
        self.X = X = rg[..., 1:J + 1]
        self.w = w = np.hanning(J + 2)[1:-1]
        self.s = s = np.sqrt(w)
        R = np.einsum("bnjr,j,bnjc->bnrc", H, w, H)
        rhs = np.einsum("bnjr,j,bnj->bnr", H, w, X)
        dt = np.dtype(dtype).type
        self.ok = np.zeros(R.shape[:2], bool)
        self.L = np.zeros_like(R)
        self.trial = np.full(R.shape[:2], TRIALS)
        for trial in range(TRIALS):
            L, ok = _cholesky(R, float(dt(eps) * dt(10**trial)))
            new = ok & ~self.ok if trials is None else ok & (trials == trial)   # `trials`: take each fit's factor at the trial given
            self.L[new], self.trial[new] = L[new], trial
            self.ok |= new
        self.L[~self.ok] = np.eye(6)
        self.a = a = np.where(self.ok[..., None], _solve(self.L, rhs), 0.0)
        self.r = r = X - np.einsum("bnjr,bnr->bnj", H, a)
        self.v, self.u = s * r, s * X
        self.numer = np.std(self.v, axis=-1, ddof=1)
        self.denom = np.std(self.u, axis=-1, ddof=1)
        self.J, self.shape = J, xb.shape
        self.A = np.where(self.ok, self.numer / (self.denom + 1e-16), upper)

    def vjp(self, gA):
        J, H, w, s, a = self.J, self.H, self.w, self.s, self.a
        live = self.ok & (self.denom > 0)
        dn = self.denom + 1e-16
        with np.errstate(all="ignore"):
            cn = np.where(live & (self.numer > 0), gA / dn / ((J - 1) * self.numer), 0.0)
            cd = np.where(live, -gA * self.numer / dn**2 / ((J - 1) * self.denom), 0.0)
        gr = s * cn[..., None] * (self.v - self.v.mean(-1, keepdims=True))
        ga = -np.einsum("bnjr,bnj->bnr", H, gr)
        z = np.where(self.ok[..., None], _solve(self.L, ga), 0.0)
        hz = np.einsum("bnjr,bnr->bnj", H, z)
        gH = (-gr - w * hz)[..., None] * a[:, :, None, :] + (w * self.r)[..., None] * z[:, :, None, :]
        gX = s * cd[..., None] * (self.u - self.u.mean(-1, keepdims=True)) + gr + w * hz
        g = np.zeros(self.shape)
        rows = np.broadcast_to(np.arange(self.shape[0])[:, None, None], gX.shape)
        for c in range(3):
            np.add.at(g, (rows, self.idx[0][..., c:c + J]), gH[..., c])
            np.add.at(g, (rows, self.idx[1][..., c:c + J]), gH[..., 3 + c])
        np.add.at(g, (rows, self.idx[2][..., 1:J + 1]), gX)
        return g


def interp_tables(sr, L, n_band):
    coarse = np.asarray([0] + [sr / 2**i for i in range(n_band, 0, -1)])
    freq = np.arange(L // 2 + 1) * (sr / L)
    idx = np.clip(np.searchsorted(coarse, freq) - 1, 0, len(coarse) - 2)
    return idx, (freq - coarse[idx]) / (coarse[idx + 1] - coarse[idx])


def aperiodicity(x, f0, P, sr, L=None, out_format=0, lower=0.001, upper=0.999, window_length_ms=30, eps=1e-5, dtype=np.float64, gy=None,
                 detail=None, trials=None):
    """x:(B, T), f0:(B, N) -> y:(B, N, K); with gy also the gradient to x.  `detail`, a dict, receives the fits.  `trials`:(n_band, B, N)
    replaces the escalation's own choice by the number of failed trials given per fit (a fit whose factor fails there counts as failed)."""
    x = np.asarray(x, np.float64)
    f0 = np.asarray(f0)
    n_band, cutoff, seg = ap_bands(sr, window_length_ms)
    bands = pyramid(x, n_band)
    fits = [Fit(bands[i], f0, P, sr, 2 * cutoff[i], seg[i], eps, upper, dtype, None if trials is None else np.asarray(trials)[i])
            for i in range(n_band)]
    if detail is not None:
        detail["fits"] = fits
    vals = np.stack([fits[-1].A] + [f.A for f in fits[::-1]], -1)   # position d: band n_band - d; position 0: the lowest band again
    if L is None:
        v, dead = vals, np.zeros(vals.shape, bool)
    else:
        idx, wgt = interp_tables(sr, L, n_band)
        v0, v1 = vals[..., idx], vals[..., idx + 1]
        dead = (v0 == 0) | (v1 == 0)
        with np.errstate(all="ignore"):
            v = np.where(dead, 0.0, np.exp((np.log(v1) - np.log(v0)) * wgt + np.log(v0)))
    c = np.clip(v, lower, upper)
    with np.errstate(all="ignore"):
        y = [c, 1 - c, c / (1 - c), (1 - c) / c][out_format]
        if gy is None:
            return y
        dconv = [np.ones_like(c), -np.ones_like(c), 1 / (1 - c)**2, -1 / c**2][out_format]
    gv = np.where(~dead & (v >= lower) & (v <= upper), np.asarray(gy, np.float64) * dconv, 0.0)
    gvals = np.zeros_like(vals)
    if L is None:
        gvals = gv
    else:
        with np.errstate(all="ignore"):
            np.add.at(gvals, (..., idx), np.where(dead, 0.0, gv * v * (1 - wgt) / v0))
            np.add.at(gvals, (..., idx + 1), np.where(dead, 0.0, gv * v * wgt / v1))
    gbands = []
    for i, f in enumerate(fits):
        gA = gvals[..., n_band - i] + (gvals[..., 0] if i == n_band - 1 else 0.0)
        gbands.append(f.vjp(gA))
    glow = gbands[-1]
    for i in range(n_band - 2, -1, -1):
        T = x.shape[1] if i == 0 else bands[i - 1].shape[1]
        glow = qmf_vjp(gbands[i], glow, T)
    return y, glow
