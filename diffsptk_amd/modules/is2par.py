"""Inverse sine coefficients -> PARCOR coefficients (reference: is2par.py): one element-wise stock operator on k_1 .. k_M, K passes through."""
from __future__ import annotations

import torch

from ..utils.private import check_size, filter_values
from .base import BaseFunctionalModule, Precomputed


class InverseSineToParcorCoefficients(BaseFunctionalModule):
    """s:(..., M+1) -> (..., M+1): k_m = sin(pi s_m / 2) (is2par.py)."""

    _takes_input_size = True

    def __init__(self, par_order: int) -> None:
        super().__init__()
        self.in_dim = par_order + 1
        self._register_precomputed(self._precompute(**filter_values(locals())))

    def forward(self, s: torch.Tensor) -> torch.Tensor:
        check_size(s.size(-1), self.in_dim, "dimension of parcor")
        return self._call_forward(s)

    @staticmethod
    def _func(x: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        pre = InverseSineToParcorCoefficients._precompute(x.size(-1) - 1, *args, **kwargs)
        return InverseSineToParcorCoefficients._apply_precomputed(pre, s=x)

    @staticmethod
    def _check(par_order: int) -> None:
        if par_order < 0:
            raise ValueError("par_order must be non-negative.")

    @staticmethod
    def _precompute(par_order: int) -> Precomputed:
        InverseSineToParcorCoefficients._check(par_order)
        return Precomputed(values={"c": torch.pi / 2})

    @staticmethod
    def _forward(s: torch.Tensor, *, c: float) -> torch.Tensor:
        K, s = torch.split(s, [1, s.size(-1) - 1], dim=-1)
        return torch.cat((K, torch.sin(c * s)), dim=-1)
