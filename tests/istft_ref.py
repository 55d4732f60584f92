"""Shared by tests/test_istft_cpu.py and tests/test_gpu_istft.py: inputs, float64 references, the comparison rule and the case tables of
the inverse path (ifftr, Unframe, ISTFT; ifftr.py:131-142, unframe.py:164-211, istft.py:186-193).

  ifftr     x[l] = sum_k c_k (Re Y_k cos(2 pi k l / n) - Im Y_k sin(2 pi k l / n)),  c_k = 1/n at k = 0 and k = n/2, 2/n in between
  unframe   x[t] = fold(y w)[t + left] / (fold(w w)[t + left] + 1e-16),  left = L // 2 if center else 0
  istft     unframe(ifftr(Y)[..., :L])

The comparison rule.  d = fold(w w) of a Blackman window is 1e-34 of its maximum at the open ends of the fold (center=False, or out_length
beyond N P): the quotient there amplifies the rounding of the numerator by 1 / (d + 1e-16).  Results are therefore compared as overlap-added
numerators: err_w[t] = |ours[t] - ref[t]| (d[t] + 1e-16) against scale = max_t |ref[t]| (d[t] + 1e-16) of the utterance, over every sample.
Cotangents of gradient tests carry the same weight (cot[t] = r[t] (d[t] + 1e-16) / max d), so that the backward's division by d + 1e-16
yields values of order r / max d everywhere and no edge sample drowns the other frames."""
import functools

import numpy as np
import torch

from oracle import oracle as O

EPS = 1e-16

# bounds, as shares of the utterance's largest entry: the ones the same kernels are held to elsewhere in the suite
B_TUNED = 2e-6        # float32, stft512_bwd_pk / stft512_bwd results and the stft512_fwd (format 5) gradient: tests/test_gpu_stft_bwd.py
B_GEN_RESULT = 2e-4   # float32 results of the generic rows: test_generic_rows_power_of_two_fft_matches_oracle_and_autograd
B_GEN_GRAD = 3e-4     # float32 gradients of the generic rows: the same test
B_F64 = 1e-9          # float64 results and gradients: the same test

PACKED, SPAN, GENERIC = "stft512_bwd_pk", "stft512_bwd", "div_rows"


def _case(route, lead, N, L, P, nfft, extra=False):
    return dict(route=route, lead=tuple(lead), N=N, L=L, P=P, nfft=nfft, extra=extra,
                id="%s-%s-N%d-L%d-P%d-n%d" % (route, "x".join(map(str, lead)), N, L, P, nfft))


# float32 geometries by the route F.istft takes for them (csrc/stft.hip, stft_bwd_impl); extra: also run with the out_length list of
# out_lengths() besides None
CASES_F32 = (
    [_case(PACKED, lead, N, 400, 80, 512, extra) for lead, N, extra in
     (((5,), 1, False), ((1,), 6, True), ((3,), 200, True), ((2,), 600, False), ((2, 5), 51, False))]
    + [_case(PACKED, lead, N, 400, 160, 512, extra) for lead, N, extra in (((5,), 1, False), ((2,), 9, True), ((3,), 100, False))]
    + [_case(SPAN, (3,), 27, L, P, 512, (L, P) == (399, 77)) for L, P in ((320, 80), (400, 100), (512, 128), (25, 10), (399, 77))]
    + [_case(GENERIC, (3,), N, L, P, nfft, nfft == 2048) for L, P, nfft, N in
       ((1200, 240, 2048, 9), (1024, 256, 1024, 9), (30, 7, 32, 29), (48, 20, 60, 11))]
)
# float64 always takes the generic rows: every geometry above with at most 27 frames
CASES_F64 = [dict(c, route=GENERIC, id="f64-" + c["id"]) for c in CASES_F32 if c["N"] <= 27]

UNFRAME_GEOMETRIES = ((400, 80), (399, 77), (30, 7))   # L = 400: the vec4 frame kernels; the others the scalar ones
UNFRAME_WINDOWS = ("blackman", "hanning", "rectangular")
UNFRAME_NORMS = ("power", "none")
UNFRAME_B, UNFRAME_N = 3, 27

IFFTR_LENGTHS = (32, 60, 512, 2048)
IFFTR_ROWS = (1, 65)


def full_length(N, L, P, center):
    return (N - 1) * P + L - (L // 2 if center else 0)


def out_lengths(c, center):
    """The out_length values a case is run with."""
    if not c["extra"]:
        return [None]
    N, P = c["N"], c["P"]
    return [None, N * P - 37, (N - 2) * P, full_length(N, c["L"], P, center), 10 ** 9, 1]


def unframe_out_lengths(L, P, center, N=UNFRAME_N):
    return [None, full_length(N, L, P, center), N * P - 37]


def ifftr_out_lengths(nfft):
    return [None, (3 * nfft) // 5, 1]


def spectra(seed, B, N, K):
    """(B, N, K) complex128, standard normal real and imaginary parts in EVERY bin: bins 0 and K - 1 carry imaginary parts, which no
    STFT of a real signal produces and which irfft ignores."""
    g = torch.Generator().manual_seed(seed)
    return torch.view_as_complex(torch.randn(B, N, K, 2, generator=g, dtype=torch.float64))


def frames(seed, B, N, L):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, N, L, generator=g, dtype=torch.float64)


@functools.lru_cache(maxsize=64)
def window64(L, window="blackman", norm="power"):
    w = O.window_table(L, window, norm, True)
    w.setflags(write=False)
    return w


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def window_sq_sum(N, L, P, center, w, out_length):
    """fold(w w), cut to the samples unframe returns (unframe.py:176-207)."""
    w = np.asarray(w, dtype=np.float64)
    den = np.zeros((N - 1) * P + L)
    for f in range(N):
        den[f * P:f * P + L] += w * w
    s = L // 2 if center else 0
    if out_length is None and center:
        out_length = N * P
    return den[s:None if out_length is None else s + out_length]


def reference(Y, L, P, nfft, center=True, window="blackman", norm="power", out_length=None):
    """(x64, d): oracle.istft of Y:(..., N, nfft/2+1) with oracle.window_table, and the overlap-added squared window of the same samples."""
    Y = _np(Y).astype(np.complex128)
    assert Y.shape[-1] == nfft // 2 + 1
    w = window64(L, window, norm)
    return O.istft(Y, L, P, center, w, out_length), window_sq_sum(Y.shape[-2], L, P, center, w, out_length)


def reference_unframe(y, P, center=True, window="rectangular", norm="none", out_length=None):
    y = _np(y).astype(np.float64)
    N, L = y.shape[-2:]
    w = window64(L, window, norm)
    return O.unframe(y, P, center, w, out_length), window_sq_sum(N, L, P, center, w, out_length)


def ifftr_torch(Yri, nfft, out_length=None):
    """irfft in plain real arithmetic, (..., K, 2) -> (..., out_length); any real dtype (float64: the reference of gradients)."""
    K = nfft // 2 + 1
    assert Yri.shape[-2:] == (K, 2)
    Lo = nfft if out_length is None else out_length
    dt = Yri.dtype
    k = torch.arange(K, dtype=torch.float64)
    c = torch.full((K,), 2.0 / nfft, dtype=torch.float64)
    c[0] = c[K - 1] = 1.0 / nfft
    ang = 2 * torch.pi * torch.outer(k, torch.arange(Lo, dtype=torch.float64)) / nfft
    sin = torch.sin(ang)
    sin[0] = sin[K - 1] = 0.0   # sin(0), sin(pi l): exactly zero, where the rounded angle leaves 1e-16 l
    return (Yri[..., 0] * c.to(dt)) @ torch.cos(ang).to(dt) - (Yri[..., 1] * c.to(dt)) @ sin.to(dt)


def unframe_torch(y, P, center, w, out_length=None):
    """fold(y w) / (fold(w w) + 1e-16) with index_add, sliced as unframe.py:176-207 slices; y:(..., N, L), w:(L,) of y's dtype."""
    N, L = y.shape[-2:]
    lead = y.shape[:-2]
    y2 = y.reshape(-1, N * L)
    full = (N - 1) * P + L
    idx = (torch.arange(N).view(N, 1) * P + torch.arange(L).view(1, L)).reshape(-1)
    num = torch.zeros(y2.shape[0], full, dtype=y.dtype).index_add(1, idx, y2 * w.repeat(N))
    den = torch.zeros(full, dtype=y.dtype).index_add(0, idx, (w * w).repeat(N))
    x = num / (den + EPS)
    s = L // 2 if center else 0
    if out_length is None and center:
        out_length = N * P
    e = full if out_length is None else s + out_length
    return x[:, s:e].reshape(*lead, -1)


def istft_torch(Yri, L, P, nfft, center=True, w=None, out_length=None):
    """The inverse STFT of the (..., N, K, 2) real view in plain real arithmetic (autograd gives the reference gradients)."""
    if w is None:
        w = torch.from_numpy(window64(L).copy()).to(Yri.dtype)
    return unframe_torch(ifftr_torch(Yri, nfft, L), P, center, w, out_length)


def weighted_ratio(ours, ref, d):
    """max over utterances of max_t |ours - ref| (d + 1e-16) / max_t |ref| (d + 1e-16); every sample counts.  ours, ref:(..., T), d:(T,)."""
    ours, ref = _np(ours).astype(np.float64), _np(ref).astype(np.float64)
    assert ours.shape == ref.shape and ref.shape[-1] == np.shape(d)[-1], (ours.shape, ref.shape, np.shape(d))
    if ref.size == 0:
        return 0.0
    wgt = np.asarray(d, dtype=np.float64) + EPS
    err = (np.abs(ours - ref) * wgt).reshape(-1, ref.shape[-1]).max(-1)
    scale = (np.abs(ref) * wgt).reshape(-1, ref.shape[-1]).max(-1)
    assert (scale > 0).all()
    r = err / scale
    return float("inf") if not np.isfinite(r).all() else float(r.max())


def relative_ratio(ours, ref, utterance_dims):
    """max over utterances of max |ours - ref| / max |ref|, an utterance being the last `utterance_dims` dimensions."""
    ours, ref = _np(ours).astype(np.float64), _np(ref).astype(np.float64)
    assert ours.shape == ref.shape, (ours.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    n = int(np.prod(ref.shape[ref.ndim - utterance_dims:]))
    err = np.abs(ours - ref).reshape(-1, n).max(-1)
    scale = np.abs(ref).reshape(-1, n).max(-1)
    assert (scale > 0).all()
    r = err / scale
    return float("inf") if not np.isfinite(r).all() else float(r.max())


def hold(label, ratio, bound):
    """Print the figure beside its bound, then assert."""
    print("[istft] %-72s ratio %.3e  bound %.1e" % (label, ratio, bound))
    assert ratio <= bound, (label, ratio, bound)
    return ratio


def worst(label, ratios, bound):
    """The closing line of a test: its largest figure beside the bound."""
    print("[istft] worst %-66s ratio %.3e  bound %.1e" % (label, max(ratios), bound))


def cotangent(seed, shape, d):
    """r[t] (d[t] + 1e-16) / max d, r standard normal: float64, shape (..., T)."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(*shape, generator=g, dtype=torch.float64)
    d = torch.as_tensor(np.asarray(d), dtype=torch.float64)
    return r * (d + EPS) / d.max()
