"""PARCOR coefficients -> log area ratio (reference: par2lar.py): one element-wise stock operator on k_1 .. k_M, K passes through."""
from __future__ import annotations

import torch

from ..utils.private import check_size, filter_values
from .base import BaseFunctionalModule, Precomputed


class ParcorCoefficientsToLogAreaRatio(BaseFunctionalModule):
    """k:(..., M+1) -> (..., M+1): g_m = 2 atanh(k_m) (par2lar.py)."""

    _takes_input_size = True

    def __init__(self, par_order: int) -> None:
        super().__init__()
        self.in_dim = par_order + 1
        self._register_precomputed(self._precompute(**filter_values(locals())))

    def forward(self, k: torch.Tensor) -> torch.Tensor:
        check_size(k.size(-1), self.in_dim, "dimension of parcor")
        return self._call_forward(k)

    @staticmethod
    def _func(x: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        pre = ParcorCoefficientsToLogAreaRatio._precompute(x.size(-1) - 1, *args, **kwargs)
        return ParcorCoefficientsToLogAreaRatio._apply_precomputed(pre, k=x)

    @staticmethod
    def _check(par_order: int) -> None:
        if par_order < 0:
            raise ValueError("par_order must be non-negative.")

    @staticmethod
    def _precompute(par_order: int) -> Precomputed:
        ParcorCoefficientsToLogAreaRatio._check(par_order)
        return Precomputed(values={"c": 2})

    @staticmethod
    def _forward(k: torch.Tensor, *, c: float) -> torch.Tensor:
        K, k = torch.split(k, [1, k.size(-1) - 1], dim=-1)
        return torch.cat((K, c * torch.atanh(k)), dim=-1)
