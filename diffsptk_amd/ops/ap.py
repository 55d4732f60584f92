"""Band aperiodicity by TANDEM-STRAIGHT (csrc/ap.hip): the QMF pyramid level by level, every (band, frame) fit of an utterance with the
interpolated, clipped output in one launch, and the adjoint down to the waveform."""
from __future__ import annotations

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ._core import _call, _dtype_code, _p, _require_device, _same_dtype, _stream

AP_FORMATS = {0: 0, "a": 0, 1: 1, "p": 1, 2: 2, "a/p": 2, 3: 3, "p/a": 3}


def ap_bands(sample_rate: int, window_length_ms: float = 30):
    """(n_band, cutoffs, segments) of ap.py:232-238, 264-266: n_band = int(log2(sample_rate / 600)) bands, the last cutoff twice."""
    n_band = 0
    while 600 << (n_band + 1) <= sample_rate:
        n_band += 1
    cutoffs = [sample_rate / 2**i for i in range(2, n_band + 1)]
    cutoffs.append(cutoffs[-1])
    return n_band, cutoffs, [int(c * window_length_ms / 500 + 1.5) for c in cutoffs]


def ap_lds_bytes(segment_sum: int, n_band: int) -> int:
    """DSA_AP_LDS_BYTES(S, n_band) of include/diffsptk_amd.h, section a25: per band five float64 arrays of J + 2 (the three runs and the
    adjoint's two), and 128 bytes for the band values and the reductions' exchange"""
    return 40 * (segment_sum + 2 * n_band) + 128


def check_ap_segments(sample_rate: int, window_length_ms: float = 30) -> None:
    """The ceiling of the per-frame workgroup, by the name of its constant; needs no device."""
    n_band, _, seg = ap_bands(sample_rate, window_length_ms)
    if n_band > _lib.AP_MAX_BANDS:
        raise ValueError(f"ap: sample_rate {sample_rate} has {n_band} bands, more than DSA_AP_MAX_BANDS = {_lib.AP_MAX_BANDS}: a wave per band")
    need = ap_lds_bytes(sum(seg), n_band)
    if need > _lib.AP_MAX_LDS_BYTES:
        raise ValueError(f"ap: the segments of sample_rate {sample_rate} and window_length_ms {window_length_ms:g} sum to {sum(seg)} samples and take "
                         f"DSA_AP_LDS_BYTES = {need} bytes per frame: the runs of every band must fit DSA_AP_MAX_LDS_BYTES = "
                         f"{_lib.AP_MAX_LDS_BYTES} bytes of LDS")


def ap_interp_tables(sample_rate: int, fft_length: int, n_band: int):
    """(segment, weight), float64 numpy of fft_length / 2 + 1 bins: the band values sit at 0 and at the band edges sample_rate / 2^i, i =
    n_band .. 1; a bin at frequency f reads the pair of edges (lower, upper] around it -- the first pair at f = 0, the last beyond the top
    edge -- with weight (f - lower) / (upper - lower) on the upper one"""
    edges = np.concatenate([[0.0], sample_rate / 2.0 ** np.arange(n_band, 0, -1)])
    f = np.arange(fft_length // 2 + 1) * (sample_rate / fft_length)
    segment = np.clip(np.searchsorted(edges, f, side="left") - 1, 0, n_band - 1)
    return segment, (f - edges[segment]) / (edges[segment + 1] - edges[segment])


def ap_windows(segments) -> np.ndarray:
    """(n_band, J_0) float64: row i holds the J_i interior points of the Hanning window of J_i + 2 points, then zeros"""
    rows = np.zeros((len(segments), max(segments)))
    for row, J in zip(rows, segments):
        row[:J] = np.hanning(J + 2)[1:-1]
    return rows


def ap_min_length(sample_rate: int) -> int:
    """The shortest waveform the pyramid takes: every level's input has at least 21 samples for the reflection pad of 20."""
    n_band, _, _ = ap_bands(sample_rate)
    return 20 * 2 ** max(n_band - 2, 0) + 1


def ap_band_lengths(T: int, n_band: int):
    """The length of every band of a waveform of T samples: each level halves, rounding up; the last band is the last level's low-pass."""
    lens, level = [], T
    for i in range(n_band):
        if i < n_band - 1:
            level = (level - 1) // 2 + 1 if level > 0 else 0
        lens.append(level)
    return lens


def _ap_pyramid(xc: torch.Tensor, n_band: int) -> torch.Tensor:
    """xc:(B, T) contiguous -> the band signals side by side, (B, sum of the band lengths), float64 whatever the data's dtype (csrc/ap.hip,
    "qmf"): band i is the high-pass of level i, the last band the last low-pass"""
    B, T = xc.shape
    code = _dtype_code(xc)
    lens = ap_band_lengths(T, n_band)
    ld = sum(lens)
    bands = torch.empty(B, ld, device=xc.device, dtype=torch.float64)
    if B:
        with torch.cuda.device(xc.device):
            level, Tl, off = xc, T, 0
            for i in range(n_band - 1):
                To = lens[i]
                last = i == n_band - 2
                low = bands[:, off + To:] if last else torch.empty(B, To, device=xc.device, dtype=torch.float64)
                # (the row stride of a contiguous level is its length: stride(0) of a one-row tensor can be anything, 0 included)
                _call("dsa_ap_qmf", _p(level), B, Tl, Tl, code if i == 0 else _lib.F64, _p(bands[:, off:]), ld, _p(low), ld if last else To,
                      _stream())
                level, Tl, off = low, To, off + To
    return bands


def ap_trials(x: torch.Tensor, f0: torch.Tensor, window: torch.Tensor, window_sqrt: torch.Tensor, cfg) -> torch.Tensor:
    """(B, N, n_band) int64: how many trials of the regulariser failed in every fit of x:(B, T), f0:(B, N) -- its m is 10^that; 9 where none
    factored.  A diagnostic: the fits run as in the backward, whose scratch records the count (header section a25); cfg as AperiodicityFn's."""
    P, sr, wms, eps, lower, upper, fmt = cfg
    check_ap_segments(sr, wms)
    n_band, _, seg = ap_bands(sr, wms)
    (B, T), N = x.shape, f0.shape[1]
    if f0.shape[0] != B or T < ap_min_length(sr):
        raise ValueError("ap_trials: x:(B, T) and f0:(B, N) must agree on B, and T must reach ap_min_length(sample_rate)")
    _same_dtype(x, f0, window, window_sqrt)
    code = _dtype_code(x)
    _require_device(x, f0, window, window_sqrt)
    fc, window, window_sqrt = f0.detach().contiguous(), window.contiguous(), window_sqrt.contiguous()
    bands = _ap_pyramid(x.detach().contiguous(), n_band)
    starts = torch.full((B, N, n_band, _lib.AP_START_WORDS), 9, device=x.device, dtype=torch.int64)
    if B and N:
        with torch.cuda.device(x.device):
            gy = torch.zeros(B, N, n_band + 1, device=x.device, dtype=x.dtype)
            gruns = torch.empty(B, N, 3 * (sum(seg) + 2 * n_band), device=x.device, dtype=x.dtype)
            gbands = torch.empty_like(bands)
            _call("dsa_ap_tandem_vjp", _p(gy), _p(bands), bands.shape[1], _p(fc), _p(window), _p(window_sqrt), window.shape[1], None, None, B, N, T, P,
                  sr, float(wms), n_band + 1, float(eps), float(lower), float(upper), fmt, code, _p(gruns), _p(starts), _p(gbands), bands.shape[1],
                  _stream())
    return starts[..., 4]


class AperiodicityFn(torch.autograd.Function):
    """x:(B, T), f0:(B, N) -> y:(B, N, K) with the module's tables (the QMF taps are the library's own float64 constants).  cfg = (P, sample_rate, window_length_ms, eps, lower, upper, format).
    Saved for the backward: the band signals, f0 and the tables; the fits are run again."""

    @staticmethod
    def forward(ctx, x, f0, window, window_sqrt, interp_indices, interp_weights, cfg):
        P, sr, wms, eps, lower, upper, fmt = cfg
        check_ap_segments(sr, wms)
        n_band, _, seg = ap_bands(sr, wms)
        B, T = x.shape
        N = f0.shape[1]
        if f0.shape[0] != B:
            raise ValueError("x and f0 must have the same batch size.")
        if T < ap_min_length(sr):
            raise ValueError(f"Input must have at least {ap_min_length(sr)} samples for sample_rate {sr}: every level of the QMF pyramid "
                             "needs 21 samples for its reflection padding.")
        _same_dtype(x, f0, window, window_sqrt, interp_weights)
        code = _dtype_code(x)
        _require_device(x, f0, window, window_sqrt, interp_indices, interp_weights)
        xc, fc = x.contiguous(), f0.detach().contiguous()
        window, window_sqrt = window.contiguous(), window_sqrt.contiguous()
        K = n_band + 1 if interp_indices is None else interp_indices.numel()
        ld = sum(ap_band_lengths(T, n_band))
        y = torch.empty(B, N, K, device=x.device, dtype=x.dtype)
        bands = _ap_pyramid(xc, n_band)
        if B and N:
            with torch.cuda.device(x.device):
                _call("dsa_ap_tandem", _p(bands), ld, _p(fc), _p(window), _p(window_sqrt), window.shape[1], _p(interp_indices),
                      _p(interp_weights), B, N, T, P, sr, float(wms), K, float(eps), float(lower), float(upper), fmt, code, _p(y), _stream())
        ctx.cfg = (cfg, T, K)
        ctx.save_for_backward(bands, fc, window, window_sqrt, interp_indices, interp_weights)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        bands, fc, window, window_sqrt, interp_indices, interp_weights = ctx.saved_tensors
        (P, sr, wms, eps, lower, upper, fmt), T, K = ctx.cfg
        n_band, _, seg = ap_bands(sr, wms)
        B, N = fc.shape
        code = _dtype_code(fc)
        lens = ap_band_lengths(T, n_band)
        ld = sum(lens)
        gx = torch.empty(B, T, device=bands.device, dtype=fc.dtype)
        if B:
            gc = gy.contiguous()
            with torch.cuda.device(bands.device):
                gbands = torch.empty_like(bands)
                gruns = torch.empty(B, N, 3 * (sum(seg) + 2 * n_band), device=bands.device, dtype=fc.dtype)
                starts = torch.empty(B, N, n_band, _lib.AP_START_WORDS, device=bands.device, dtype=torch.int64)
                _call("dsa_ap_tandem_vjp", _p(gc), _p(bands), ld, _p(fc), _p(window), _p(window_sqrt), window.shape[1], _p(interp_indices),
                      _p(interp_weights), B, N, T, P, sr, float(wms), K, float(eps), float(lower), float(upper), fmt, code, _p(gruns), _p(starts),
                      _p(gbands), ld, _stream())
                # the pyramid's transpose from the deepest level up: level i's input gathers band i and the level below
                offs = [sum(lens[:i]) for i in range(n_band)]
                glow, ldlow = gbands[:, offs[-1]:], ld
                for i in range(n_band - 2, -1, -1):
                    Tl = T if i == 0 else lens[i - 1]
                    gin = gx if i == 0 else torch.empty(B, Tl, device=bands.device, dtype=torch.float64)
                    _call("dsa_ap_qmf_vjp", _p(gbands[:, offs[i]:]), ld, _p(glow), ldlow, B, Tl, code if i == 0 else _lib.F64, _p(gin), Tl, _stream())
                    glow, ldlow = gin, Tl
        return gx, None, None, None, None, None, None
