"""Decimation and Interpolation (reference: decimate.py, interpolate.py): the resampling around the pseudo-QMF banks.  Decimation
is a view, as in the reference; Interpolation is one scatter launch (csrc/pqmf.hip).  Next to a bank, fuse() folds either into the
bank's launch (modules/fused.py)."""
from __future__ import annotations

import torch

from .. import ops
from ..utils.private import filter_values
from .base import BaseFunctionalModule, Precomputed


class Decimation(BaseFunctionalModule):
    """x:(..., T, ...) -> the view x[..., start::period, ...] along dim (decimate.py:88-93)."""

    def __init__(self, period: int, start: int = 0, dim: int = -1) -> None:
        super().__init__()
        self._register_precomputed(self._precompute(**filter_values(locals())))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._call_forward(x)

    @staticmethod
    def _func(x: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        pre = Decimation._precompute(*args, **kwargs)
        return Decimation._apply_precomputed(pre, x=x)

    @staticmethod
    def _check(period: int, start: int, dim: int) -> None:
        if period <= 0:
            raise ValueError("period must be positive.")
        if start < 0:
            raise ValueError("start must be non-negative.")

    @staticmethod
    def _precompute(period: int, start: int, dim: int) -> Precomputed:
        Decimation._check(period, start, dim)
        return Precomputed(values={"period": period, "start": start, "dim": dim})

    @staticmethod
    def _forward(x: torch.Tensor, *, period: int, start: int, dim: int) -> torch.Tensor:
        if not -x.ndim <= dim < x.ndim:
            raise ValueError(f"Dimension {dim} out of range.")
        dim = dim % x.ndim
        return x[(slice(None),) * dim + (slice(start, None, period),)]


class Interpolation(BaseFunctionalModule):
    """x:(..., T, ...) -> (..., T period + start, ...) along dim: zeros, with x[n] at start + n period (interpolate.py:85-96)."""

    def __init__(self, period: int, start: int = 0, dim: int = -1) -> None:
        super().__init__()
        self._register_precomputed(self._precompute(**filter_values(locals())))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._call_forward(x)

    @staticmethod
    def _func(x: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        pre = Interpolation._precompute(*args, **kwargs)
        return Interpolation._apply_precomputed(pre, x=x)

    @staticmethod
    def _check(period: int, start: int, dim: int) -> None:
        Decimation._check(period, start, dim)

    @staticmethod
    def _precompute(period: int, start: int, dim: int) -> Precomputed:
        return Decimation._precompute(period, start, dim)

    @staticmethod
    def _forward(x: torch.Tensor, *, period: int, start: int, dim: int) -> torch.Tensor:
        if not -x.ndim <= dim < x.ndim:
            raise ValueError(f"Dimension {dim} out of range.")
        return ops.InterpolateFn.apply(x, period, start, dim)
