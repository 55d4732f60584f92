"""Line spectral pairs -> LPC coefficients (reference: lsp2lpc.py): products of real second-order sections, one launch forward and
one backward (csrc/lsp.hip); no complex arithmetic, and no order or dtype at which it refuses."""
from __future__ import annotations

import torch

from .. import ops
from ..utils.private import check_size, filter_values
from .base import BaseFunctionalModule, Precomputed
from .lpc2lsp import lsp_unit


class LineSpectralPairsToLinearPredictiveCoefficients(BaseFunctionalModule):
    """w:(..., M+1) = [K, w_1 .. w_M] -> a:(..., M+1) = [K, a_1 .. a_M] (lsp2lpc.py:171-195)."""

    _takes_input_size = True

    def __init__(self, lpc_order: int, log_gain: bool = False, sample_rate: int | None = None, in_format: str | int = "radian",
                 device: torch.device | None = None, dtype: torch.dtype | None = None) -> None:
        super().__init__()
        self.in_dim = lpc_order + 1
        self._register_precomputed(self._precompute(**filter_values(locals())))

    def forward(self, w: torch.Tensor) -> torch.Tensor:
        check_size(w.size(-1), self.in_dim, "dimension of LSP")
        return self._call_forward(w)

    @staticmethod
    def _func(w: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        pre = LineSpectralPairsToLinearPredictiveCoefficients._precompute(w.size(-1) - 1, *args, **kwargs, device=w.device, dtype=w.dtype)
        return LineSpectralPairsToLinearPredictiveCoefficients._apply_precomputed(pre, w=w)

    @staticmethod
    def _check(lpc_order: int, log_gain: bool, sample_rate: int | None, in_format: str | int) -> None:
        if lpc_order < 0:
            raise ValueError("lpc_order must be non-negative.")
        if in_format in (2, 3, "hz", "khz") and (sample_rate is None or sample_rate <= 0):
            raise ValueError("sample_rate must be positive.")

    @staticmethod
    def _precompute(lpc_order: int, log_gain: bool, sample_rate: int | None, in_format: str | int,
                    device: torch.device | None = None, dtype: torch.dtype | None = None) -> Precomputed:
        LineSpectralPairsToLinearPredictiveCoefficients._check(lpc_order, log_gain, sample_rate, in_format)
        return Precomputed(values={"log_gain": log_gain, "unit": lsp_unit(in_format, sample_rate, "in_format")})

    @staticmethod
    def _forward(w: torch.Tensor, *, log_gain: bool, unit: float) -> torch.Tensor:
        return ops.lsp2lpc(w, log_gain, unit)
