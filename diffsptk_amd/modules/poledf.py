"""Time-variant all-pole (LPC synthesis) filter (reference: poledf.py) -- the synthesis side of the LPC branch: the output
[K, a_1 .. a_M] of LPC is its coefficient input."""
from __future__ import annotations

import torch

from .. import ops
from ..utils.private import check_size, filter_values
from .base import BaseFunctionalModule, Precomputed


class AllPoleDigitalFilter(BaseFunctionalModule):
    """x:(..., T), a:(..., T/P, M+1) -> y:(..., T):  y[t] = K_t x[t] - sum_{k=1..M} a_t[k] y[t - k], zero initial state, with
    [K_t, a_t] interpolated linearly between frames (poledf.py:117-140 with torchlpc.sample_wise_lpc).  The recursion runs in one
    wave per utterance (csrc/poledf.hip), forward and backward."""

    _takes_input_size = True

    def __init__(self, filter_order: int, frame_period: int, ignore_gain: bool = False) -> None:
        super().__init__()
        self.in_dim = filter_order + 1
        self._register_precomputed(self._precompute(**filter_values(locals())))

    def forward(self, x: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
        check_size(a.size(-1), self.in_dim, "dimension of LPC coefficients")
        return self._call_forward(x, a)

    @staticmethod
    def _func(x: torch.Tensor, a: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        pre = AllPoleDigitalFilter._precompute(a.size(-1) - 1, *args, **kwargs)
        return AllPoleDigitalFilter._apply_precomputed(pre, x=x, a=a)

    @staticmethod
    def _check(filter_order: int, frame_period: int) -> None:
        if filter_order < 0:
            raise ValueError("filter_order must be non-negative.")
        if frame_period <= 0:
            raise ValueError("frame_period must be positive.")

    @staticmethod
    def _precompute(filter_order: int, frame_period: int, ignore_gain: bool = False) -> Precomputed:
        AllPoleDigitalFilter._check(filter_order, frame_period)
        return Precomputed(values={"frame_period": frame_period, "ignore_gain": ignore_gain})

    @staticmethod
    def _forward(x: torch.Tensor, a: torch.Tensor, *, frame_period: int, ignore_gain: bool) -> torch.Tensor:
        check_size(x.size(-1), a.size(-2) * frame_period, "sequence length")
        d = x.dim()
        if d == 1:
            x, a = x.unsqueeze(0), a.unsqueeze(0)
        if a.dim() > 3:   # the reference's interpolation (linear_intpl.py:104) takes at most (B, N, M+1)
            raise ValueError("Input must be 1D, 2D, or 3D tensor.")
        y = ops.poledf(x, a, frame_period, ignore_gain)
        return y.squeeze(0) if d == 1 else y
