"""Stability check of line spectral pairs (reference: lspcheck.py): the Gauss-Seidel sweeps that push adjacent LSPs apart and the
clip into (0, pi) -- one launch forward and one backward (csrc/lsp.hip)."""
from __future__ import annotations

import math
import warnings

import torch

from .. import ops
from ..utils.private import check_size, filter_values
from .base import BaseFunctionalModule, Precomputed


class LineSpectralPairsStabilityCheck(BaseFunctionalModule):
    """w:(..., M+1) -> the LSPs at least rate pi / (M + 1) apart and inside [that, pi - that] after n_iter sweeps (lspcheck.py:115-145).
    Each row stops sweeping on its own distances (the reference's break is batch-wide): a row's result does not depend on the batch.
    warn_type "ignore" never synchronises (it runs under graph capture); "warn" and "exit" read one flag back from the device, as
    the reference's torch.any does."""

    _takes_input_size = True

    def __init__(self, lsp_order: int, rate: float = 0, n_iter: int = 1, warn_type: str = "warn") -> None:
        super().__init__()
        self.in_dim = lsp_order + 1
        self._register_precomputed(self._precompute(**filter_values(locals())))

    def forward(self, w: torch.Tensor) -> torch.Tensor:
        check_size(w.size(-1), self.in_dim, "dimension of LSP")
        return self._call_forward(w)

    @staticmethod
    def _func(w: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        pre = LineSpectralPairsStabilityCheck._precompute(w.size(-1) - 1, *args, **kwargs)
        return LineSpectralPairsStabilityCheck._apply_precomputed(pre, w=w)

    @staticmethod
    def _check(lsp_order: int, rate: float, n_iter: int) -> None:
        if lsp_order < 0:
            raise ValueError("lsp_order must be non-negative.")
        if not 0 <= rate <= 1:
            raise ValueError("rate must be in [0, 1].")
        if n_iter < 0:
            raise ValueError("n_iter must be non-negative.")

    @staticmethod
    def _precompute(lsp_order: int, rate: float, n_iter: int, warn_type: str) -> Precomputed:
        LineSpectralPairsStabilityCheck._check(lsp_order, rate, n_iter)
        return Precomputed(values={"min_distance": rate * math.pi / (lsp_order + 1), "n_iter": n_iter, "warn_type": warn_type})

    @staticmethod
    def _forward(w: torch.Tensor, *, min_distance: float, n_iter: int, warn_type: str) -> torch.Tensor:
        out, unstable = ops.lspcheck(w, min_distance, n_iter, detect=warn_type != "ignore")
        if unstable is not None and unstable.item():
            if warn_type == "warn":
                warnings.warn("Detected unstable LSP coefficients.")
            elif warn_type == "exit":
                raise RuntimeError("Detected unstable LSP coefficients.")
            else:
                raise RuntimeError
        return out
