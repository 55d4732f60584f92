"""Log area ratio -> PARCOR coefficients (reference: lar2par.py): one element-wise stock operator on k_1 .. k_M, K passes through."""
from __future__ import annotations

import torch

from ..utils.private import check_size, filter_values
from .base import BaseFunctionalModule, Precomputed


class LogAreaRatioToParcorCoefficients(BaseFunctionalModule):
    """g:(..., M+1) -> (..., M+1): k_m = tanh(g_m / 2) (lar2par.py)."""

    _takes_input_size = True

    def __init__(self, par_order: int) -> None:
        super().__init__()
        self.in_dim = par_order + 1
        self._register_precomputed(self._precompute(**filter_values(locals())))

    def forward(self, g: torch.Tensor) -> torch.Tensor:
        check_size(g.size(-1), self.in_dim, "dimension of parcor")
        return self._call_forward(g)

    @staticmethod
    def _func(x: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        pre = LogAreaRatioToParcorCoefficients._precompute(x.size(-1) - 1, *args, **kwargs)
        return LogAreaRatioToParcorCoefficients._apply_precomputed(pre, g=x)

    @staticmethod
    def _check(par_order: int) -> None:
        if par_order < 0:
            raise ValueError("par_order must be non-negative.")

    @staticmethod
    def _precompute(par_order: int) -> Precomputed:
        LogAreaRatioToParcorCoefficients._check(par_order)
        return Precomputed(values={"c": 0.5})

    @staticmethod
    def _forward(g: torch.Tensor, *, c: float) -> torch.Tensor:
        K, g = torch.split(g, [1, g.size(-1) - 1], dim=-1)
        return torch.cat((K, torch.tanh(c * g)), dim=-1)
