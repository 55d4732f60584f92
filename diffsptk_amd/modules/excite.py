"""Excitation generation (reference: excite.py): pitch in samples, 0 = unvoiced, to the signal that drives a synthesis filter.  The voiced
part -- interpolated pitch, its reciprocal, the float64 phase sum that restarts at every voiced run, the shape on that phase -- is one
launch (csrc/excite.hip); the unvoiced part is torch's generator and one select.

Departures from the reference (include/diffsptk_amd.h, section a17):
  * the caller's tensor is not modified (the reference overwrites p in place at every voiced-to-unvoiced boundary);
  * the result is an ordinary tensor without a gradient (the reference returns an inference tensor, which MLSA cannot save for its
    backward pass);
  * pitch values that are negative or in (0, 1) are outside the contract;
  * the interpolated pitch is a + w (b - a) as in this library's filters; it differs from F.interpolate in the last place on some samples;
  * "gauss" and "uniform" draw noise for EVERY sample on the device and keep it where the frame is unvoiced: no count is read back, so
    the call can be captured in a graph, and for one seed the values differ from the reference's, which draws as many numbers as there
    are unvoiced samples.
"m-sequence" lays one M-sequence over the unvoiced samples of the whole batch in flattened order, as the reference does, and is the one
option that reads a count back to the host.

The class is exported from the package root and through functional.excite, not from diffsptk_amd.modules, for the reason given in
modules/mlsacheck.py."""
from __future__ import annotations

import functools
import math

import torch

from .. import ops
from ..signals import mseq
from ..utils.private import filter_values
from .base import BaseFunctionalModule, Precomputed

_VOICED = ("pulse", "harmonic-pulse", "sinusoidal", "sawtooth", "inverted-sawtooth", "triangle", "square")
_UNVOICED = ("zeros", "gauss", "m-sequence", "uniform")


@functools.lru_cache(maxsize=8)
def _mseq_table(length: int) -> torch.Tensor:
    """mseq of `length` values on the host, in float64 (+-1 is exact in every dtype)."""
    return mseq(length - 1, dtype=torch.float64)


class ExcitationGeneration(BaseFunctionalModule):
    """p:(..., N) -> (..., N P) (excite.py:222-310).  voiced_region: "pulse", "harmonic-pulse", "sinusoidal", "sawtooth",
    "inverted-sawtooth", "triangle" or "square"; unvoiced_region: "zeros", "gauss", "m-sequence" or "uniform"; polarity: "auto"
    (unipolar for "pulse", else bipolar), "unipolar" or "bipolar"; init_phase: "zeros", "random" (one draw per utterance) or radians."""

    def __init__(
        self,
        frame_period: int,
        *,
        voiced_region: str = "pulse",
        unvoiced_region: str = "gauss",
        polarity: str = "auto",
        init_phase: str | float = "zeros",
    ) -> None:
        super().__init__()
        self._register_precomputed(self._precompute(**filter_values(locals())))

    def forward(self, p: torch.Tensor) -> torch.Tensor:
        return self._call_forward(p)

    @staticmethod
    def _func(x: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        pre = ExcitationGeneration._precompute(*args, **kwargs)
        return ExcitationGeneration._apply_precomputed(pre, p=x)

    @staticmethod
    def _check(frame_period: int) -> None:
        if frame_period <= 0:
            raise ValueError("frame_period must be positive.")

    @staticmethod
    def _precompute(frame_period: int, voiced_region: str, unvoiced_region: str, polarity: str, init_phase: str | float) -> Precomputed:
        ExcitationGeneration._check(frame_period)
        return Precomputed(values={"frame_period": frame_period, "voiced_region": voiced_region, "unvoiced_region": unvoiced_region,
                                   "polarity": polarity, "init_phase": init_phase})

    @staticmethod
    def _forward(p: torch.Tensor, *, frame_period: int, voiced_region: str, unvoiced_region: str, polarity: str,
                 init_phase: str | float) -> torch.Tensor:
        # the reference's checks in the reference's order (linear_intpl.py:86-95, excite.py:250-307), all before anything runs
        if frame_period != 1 and p.dim() > 3:
            raise ValueError("Input must be 1D, 2D, or 3D tensor.")
        if isinstance(init_phase, str) and init_phase not in ("zeros", "random"):
            raise ValueError(f"init_phase {init_phase} is not supported.")
        if polarity not in ("auto", "unipolar", "bipolar"):
            raise ValueError(f"polarity {polarity} is not supported.")
        if voiced_region not in _VOICED:
            raise ValueError(f"voiced_region {voiced_region} is not supported.")
        if unvoiced_region not in _UNVOICED:
            raise ValueError(f"unvoiced_region {unvoiced_region} is not supported.")
        bipolar = voiced_region != "pulse" if polarity == "auto" else polarity == "bipolar"

        with torch.no_grad():
            p = p.detach()
            if not isinstance(init_phase, str):
                shift = init_phase / math.tau
            elif init_phase == "zeros":
                shift = 0.0
            else:
                ops._require_device(p)
                shift = torch.rand(p.shape[:-1], device=p.device, dtype=p.dtype)
            e = ops.excite(p, frame_period, voiced_region, bipolar, shift)
            if unvoiced_region == "zeros":
                return e
            voiced = (p != 0).unsqueeze(-1).expand(*p.shape, frame_period).reshape(e.shape)
            if unvoiced_region == "gauss":
                return torch.where(voiced, e, torch.randn_like(e))
            if unvoiced_region == "uniform":
                return torch.where(voiced, e, math.sqrt(12) * torch.rand_like(e))   # (not centred: excite.py:125-126)
            unvoiced = ~voiced
            count = int(unvoiced.sum())   # the one host read of this module
            if count:
                e.masked_scatter_(unvoiced, _mseq_table(count).to(device=e.device, dtype=e.dtype))
            return e
