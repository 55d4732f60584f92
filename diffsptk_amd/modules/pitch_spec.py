"""PitchAdaptiveSpectralAnalysis (reference: pitch_spec.py): a waveform and its F0 to the spectral envelope of CheapTrick, the `sp` that
WorldSynthesis takes.  Forward (csrc/pitch_spec.hip): ONE launch, one workgroup per frame -- the pitch-adaptive window, the power spectrum,
the DC correction, the linear smoothing, the liftering through two more transforms and the output format without leaving LDS; backward:
the frames' adjoint and a gather, two launches.  The gradient flows to `x`; none to `f0` (the reference detaches it).

Departures from the reference (include/diffsptk_amd.h, section a26):
  * algorithm="straight" raises ValueError saying that only "cheap-trick" is built (STRAIGHT needs scipy and pylstraight and is
    float64-only); an unknown name keeps the reference's "is not supported" text;
  * fft_length must be a power of two (the reference accepts any length >= 1024; WORLD itself only uses powers of two), and the per-frame
    workgroup must fit DSA_PITCH_SPEC_LDS_BYTES(L) <= DSA_PITCH_SPEC_MAX_LDS_BYTES = 163840: fft_length <= 4096, which serves 96 kHz.
    Anything else raises ValueError naming the constant, at construction, before a device is needed;
  * everything from the loaded sample to the formatted value runs in float64 for both dtypes, and a float32 call returns the float64
    result rounded once.  The reference's float32 result is about 1e-3 off its own float64 result on a log spectrum of magnitude 5 (the
    smoothing is the difference of two float32 running sums);
  * the floor noise of step "AddInfinitesimalNoise" is |randn| 2^-52, finfo(float64).eps, for both dtypes, because the arithmetic it protects
    is float64 for both.  The reference's float32 run adds |randn| 2^-23, which alone moves its result by 1e-5 .. 3e-4 of the largest
    value; a float32 call here is the float64 call's result rounded once, with the same noise rows;
  * the running sum of the smoothing starts at the frame's own boundary.  The reference pads every frame by the widest boundary of the
    batch -- its one host read, int(torch.amax(boundary)) -- so there a frame's last bits depend on its neighbours.  Here a frame's bits
    are those of the frame run alone, given the same noise rows, and there is no host read anywhere: the module is capturable by Graphed;
  * the noise comes from the overridable `self._randn(shape)`: torch's generator on the module's device.  The same seed gives different noise from the
    reference's CPU generator;
  * f0 must have (T - 1) // frame_period + 1 frames (ValueError naming both numbers; the reference fails in a broadcast), and x and f0
    must agree on the batch size.

The integers -- the window's half length round(1.5 sr / f), the bins of the DC correction, the truncations of the linear reads, f0 <= f_min
-- are evaluated in float64 from the stored values.  The reads are continuous across their truncations; the window's edge and the DC mask
are not, so a float32 reference run can choose differently within a rounding of a tie.

The class is exported from the package root, not from diffsptk_amd.modules, for the reason given in modules/mlsacheck.py; there is no
functional form because the reference has none."""
from __future__ import annotations

import math

import numpy as np
import torch
from torch import nn

from .. import ops
from .spec import Spectrum, device_twiddle


def _rows(t: torch.Tensor) -> torch.Tensor:
    """(..., n) as (rows, n); an empty batch keeps its n"""
    return t.reshape(math.prod(t.shape[:-1]), t.shape[-1])


class SpectrumExtractionByCheapTrick(nn.Module):
    """The extractor of the reference (pitch_spec.py:206-255): its constants, its inner `spec` module and its non-persistent `ramp`."""

    def __init__(
        self,
        frame_period: int,
        sample_rate: int,
        fft_length: int,
        *,
        default_f0: float = 500,
        q1: float = -0.15,
        eps: float = 0,
        relative_floor: float | None = None,
        device: torch.device | None = None,
        dtype: torch.dtype | None = None,
    ) -> None:
        super().__init__()

        self.frame_period = frame_period
        self.sample_rate = sample_rate
        self.fft_length = fft_length

        # GetF0FloorForCheapTrick()
        self.f_min = 3 * sample_rate / (fft_length - 3)
        if default_f0 < self.f_min:
            raise ValueError(f"default_f0 must be at least {self.f_min}.")

        # GetFFTSizeForCheapTrick()
        min_fft_length = 2 ** (1 + int(np.log(3 * sample_rate / self.f_min + 1) / np.log(2)))
        if fft_length < min_fft_length:
            raise ValueError(f"fft_length must be at least {min_fft_length}.")

        self.q1 = q1
        self.default_f0 = default_f0

        self.spec = Spectrum(fft_length, eps=eps, relative_floor=relative_floor, out_format="power")
        self.eps = eps
        self.relative_floor = relative_floor

        self.register_buffer("ramp", torch.arange(fft_length, device=device, dtype=dtype), persistent=False)

    def _randn(self, shape) -> torch.Tensor:
        """Every random draw of `forward`: standard normal numbers from torch's generator of the module's device (torch.manual_seed
        seeds it), float32 unless the module's dtype is float64."""
        dtype = self.ramp.dtype if self.ramp.dtype.is_floating_point else torch.get_default_dtype()
        return torch.randn(*shape, device=self.ramp.device, dtype=dtype)

    def forward(self, x: torch.Tensor, f0: torch.Tensor) -> torch.Tensor:
        """x:(..., T), f0:(..., N) -> (..., N, L/2+1): the log power spectrum (twice the log-magnitude, exactly)"""
        lead = x.shape[:-1]
        sp = 2 * self._analyse(_rows(x), _rows(f0), ops.PITCH_SPEC_FORMATS["log-magnitude"])
        return sp.reshape(*lead, *sp.shape[1:])

    def _analyse(self, x: torch.Tensor, f0: torch.Tensor, out_format: int, randn=None) -> torch.Tensor:
        """the envelope in out_format 0 .. 3, formatted in the same launch; randn: whose draws to take (the outer module's)"""
        randn = randn or self._randn
        B, N = f0.shape
        L = self.fft_length
        floor_ratio = 0.0 if self.relative_floor is None else 10 ** (self.relative_floor / 10)
        cfg = (self.frame_period, self.sample_rate, L, self.default_f0, self.q1, self.eps, floor_ratio, out_format)
        noise1 = randn((B, N, L)).to(x.dtype)
        noise2 = randn((B, N, L // 2 + 1)).to(x.dtype)
        return ops.PitchSpecFn.apply(x, f0, noise1, noise2, device_twiddle(L, x.device, torch.float64), cfg)


class PitchAdaptiveSpectralAnalysis(nn.Module):
    """(x:(..., T), f0:(..., N) in Hz, N = (T - 1) // P + 1) -> (..., N, L/2+1) (pitch_spec.py:39-168).
    frame_period >= 1, sample_rate >= 8000, fft_length >= 1024 and a power of two, algorithm "cheap-trick", out_format "db",
    "log-magnitude", "magnitude" or "power" (or 0 .. 3); keywords default_f0, q1, eps, relative_floor, device, dtype."""

    def __init__(
        self,
        frame_period: int,
        sample_rate: int,
        fft_length: int,
        algorithm: str = "cheap-trick",
        out_format: str | int = "power",
        **kwargs,
    ) -> None:
        super().__init__()

        if frame_period <= 0:
            raise ValueError("frame_period must be positive.")
        if sample_rate < 8000:
            raise ValueError("sample_rate must be at least 8000 Hz.")
        if fft_length < 1024:
            raise ValueError("fft_length must be at least 1024.")
        ops.check_pitch_spec_length(fft_length)

        if algorithm == "cheap-trick":
            self.extractor = SpectrumExtractionByCheapTrick(frame_period, sample_rate, fft_length, **kwargs)
        elif algorithm == "straight":
            raise ValueError("algorithm straight is not built: diffsptk_amd has only the cheap-trick algorithm.")
        else:
            raise ValueError(f"algorithm {algorithm} is not supported.")

        if out_format not in ops.PITCH_SPEC_FORMATS or isinstance(out_format, bool):
            raise ValueError(f"out_format {out_format} is not supported.")
        self.out_format = ops.PITCH_SPEC_FORMATS[out_format]

    def _randn(self, shape) -> torch.Tensor:
        """Every random draw of `forward` (the frame's noise, then the floor noise): override it to supply the noise."""
        return self.extractor._randn(shape)

    def forward(self, x: torch.Tensor, f0: torch.Tensor) -> torch.Tensor:
        if x.dim() == 0 or f0.dim() != x.dim() or f0.shape[:-1] != x.shape[:-1]:
            raise ValueError("x:(..., T) and f0:(..., N) must have the same leading dimensions.")
        lead = x.shape[:-1]
        sp = self.extractor._analyse(_rows(x), _rows(f0), self.out_format, self._randn)
        return sp.reshape(*lead, *sp.shape[1:])
