"""Stability check of LPC coefficients (reference: lpccheck.py): step-down, clip the PARCOR coefficients, step-up -- one launch
forward and one backward (csrc/parcor.hip)."""
from __future__ import annotations

import warnings

import torch

from .. import ops
from ..utils.private import check_size, filter_values
from .base import BaseFunctionalModule, Precomputed


class LinearPredictiveCoefficientsStabilityCheck(BaseFunctionalModule):
    """a:(..., M+1) -> the coefficients with every |k_m| clipped to 1 - margin (lpccheck.py:104-121).  warn_type "ignore" never
    synchronises (it runs under graph capture); "warn" and "exit" read one flag back from the device, as the reference's
    torch.any does."""

    _takes_input_size = True

    def __init__(self, lpc_order: int, margin: float = 1e-16, warn_type: str = "warn") -> None:
        super().__init__()
        self.in_dim = lpc_order + 1
        self._register_precomputed(self._precompute(**filter_values(locals())))

    def forward(self, a: torch.Tensor) -> torch.Tensor:
        check_size(a.size(-1), self.in_dim, "dimension of LPC")
        return self._call_forward(a)

    @staticmethod
    def _func(a: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        pre = LinearPredictiveCoefficientsStabilityCheck._precompute(a.size(-1) - 1, *args, **kwargs)
        return LinearPredictiveCoefficientsStabilityCheck._apply_precomputed(pre, a=a)

    @staticmethod
    def _check(lpc_order: int, margin: float) -> None:
        if lpc_order < 0:
            raise ValueError("lpc_order must be non-negative.")
        if not 0 < margin < 1:
            raise ValueError("margin must be in (0, 1).")

    @staticmethod
    def _precompute(lpc_order: int, margin: float, warn_type: str) -> Precomputed:
        LinearPredictiveCoefficientsStabilityCheck._check(lpc_order, margin)
        return Precomputed(values={"bound": 1 - margin, "warn_type": warn_type})

    @staticmethod
    def _forward(a: torch.Tensor, *, bound: float, warn_type: str) -> torch.Tensor:
        out, unstable = ops.lpccheck(a, bound, detect=warn_type != "ignore")
        if unstable is not None and unstable.item():
            if warn_type == "warn":
                warnings.warn("Detected unstable LPC coefficients.")
            elif warn_type == "exit":
                raise RuntimeError("Detected unstable LPC coefficients.")
            else:
                raise RuntimeError
        return out
