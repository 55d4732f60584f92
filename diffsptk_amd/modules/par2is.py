"""PARCOR coefficients -> inverse sine coefficients (reference: par2is.py): one element-wise stock operator on k_1 .. k_M, K passes through."""
from __future__ import annotations

import torch

from ..utils.private import check_size, filter_values
from .base import BaseFunctionalModule, Precomputed


class ParcorCoefficientsToInverseSine(BaseFunctionalModule):
    """k:(..., M+1) -> (..., M+1): s_m = (2 / pi) asin(clip(k_m, +-(1 - 1e-6))) (par2is.py)."""

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
        pre = ParcorCoefficientsToInverseSine._precompute(x.size(-1) - 1, *args, **kwargs)
        return ParcorCoefficientsToInverseSine._apply_precomputed(pre, k=x)

    @staticmethod
    def _check(par_order: int) -> None:
        if par_order < 0:
            raise ValueError("par_order must be non-negative.")

    @staticmethod
    def _precompute(par_order: int) -> Precomputed:
        ParcorCoefficientsToInverseSine._check(par_order)
        return Precomputed(values={"c": 2 / torch.pi})

    @staticmethod
    def _forward(k: torch.Tensor, *, c: float) -> torch.Tensor:
        K, k = torch.split(k, [1, k.size(-1) - 1], dim=-1)
        eps = 1e-6
        k = torch.clip(k, min=-1 + eps, max=1 - eps)
        return torch.cat((K, c * torch.asin(k)), dim=-1)
