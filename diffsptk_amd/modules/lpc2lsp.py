"""LPC coefficients -> line spectral pairs (reference: lpc2lsp.py): a root search on two Chebyshev series after Kabal and
Ramachandran, one launch forward and one backward (csrc/lsp.hip); no eigen-solver."""
from __future__ import annotations

import math

import torch

from .. import ops
from ..utils.private import check_size, filter_values
from .base import BaseFunctionalModule, Precomputed


def lsp_unit(fmt: str | int, sample_rate: int | None, name: str) -> float:
    """Radians per unit of an LSP format (lpc2lsp.py:136-145, lsp2lpc.py:128-145)."""
    if fmt in (0, "radian"):
        return 1.0
    if fmt in (1, "cycle"):
        return math.tau
    if fmt in (2, "khz"):
        return math.tau / sample_rate * 1000
    if fmt in (3, "hz"):
        return math.tau / sample_rate
    raise ValueError(f"{name} {fmt} is not supported.")


class LinearPredictiveCoefficientsToLineSpectralPairs(BaseFunctionalModule):
    """a:(..., M+1) = [K, a_1 .. a_M] -> w:(..., M+1) = [K, w_1 .. w_M], 0 < w_1 < .. < w_M < pi in radians (lpc2lsp.py:169-197).  A row
    that is no minimum-phase predictor comes back as NaN in w_1 .. w_M (the reference returns the angles of off-circle roots): run
    lpccheck first where that can happen."""

    _takes_input_size = True

    def __init__(self, lpc_order: int, log_gain: bool = False, sample_rate: int | None = None, out_format: str | int = "radian",
                 device: torch.device | None = None, dtype: torch.dtype | None = None) -> None:
        super().__init__()
        self.in_dim = lpc_order + 1
        self._register_precomputed(self._precompute(**filter_values(locals())))

    def forward(self, a: torch.Tensor) -> torch.Tensor:
        check_size(a.size(-1), self.in_dim, "dimension of LPC")
        return self._call_forward(a)

    @staticmethod
    def _func(a: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        pre = LinearPredictiveCoefficientsToLineSpectralPairs._precompute(a.size(-1) - 1, *args, **kwargs, device=a.device, dtype=a.dtype)
        return LinearPredictiveCoefficientsToLineSpectralPairs._apply_precomputed(pre, a=a)

    @staticmethod
    def _check(lpc_order: int, log_gain: bool, sample_rate: int | None, out_format: str | int) -> None:
        if lpc_order < 0:
            raise ValueError("lpc_order must be non-negative.")
        if out_format in (2, 3, "hz", "khz") and (sample_rate is None or sample_rate <= 0):
            raise ValueError("sample_rate must be positive.")

    @staticmethod
    def _precompute(lpc_order: int, log_gain: bool, sample_rate: int | None, out_format: str | int,
                    device: torch.device | None = None, dtype: torch.dtype | None = None) -> Precomputed:
        LinearPredictiveCoefficientsToLineSpectralPairs._check(lpc_order, log_gain, sample_rate, out_format)
        return Precomputed(values={"log_gain": log_gain, "unit": lsp_unit(out_format, sample_rate, "out_format")})

    @staticmethod
    def _forward(a: torch.Tensor, *, log_gain: bool, unit: float) -> torch.Tensor:
        return ops.lpc2lsp(a, log_gain, unit)[0]
