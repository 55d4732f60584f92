"""Delta features (reference: delta.py): the static components and their regression windows in one launch (csrc/paramgen.hip).

The class is exported from the package root and through functional.delta, not yet from diffsptk_amd.modules: the alignment sweep's
table (tests/alignment_rows.py) has a row per name of modules.__all__, and its row arrives with the change that may edit that table."""
from __future__ import annotations

import torch

from .. import ops
from ..utils import tables
from ..utils.private import filter_values, to
from .base import BaseFunctionalModule, Precomputed


class Delta(BaseFunctionalModule):
    """x:(B, T, D) or (T, D) -> (B, T, D H) or (T, D H): per window h the D components, the windows applied along T with the first and
    last frame repeated (delta.py:181-201).  seed: lists of delta coefficients, or the width(s) of the first (and second) order
    regression coefficients; static_out=False leaves the static components out."""

    def __init__(
        self,
        seed=[[-0.5, 0, 0.5], [1, -2, 1]],
        static_out: bool = True,
        device: torch.device | None = None,
        dtype: torch.dtype | None = None,
    ) -> None:
        super().__init__()
        self._register_precomputed(self._precompute(**filter_values(locals())))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._call_forward(x)

    @staticmethod
    def _func(x: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        _p = Delta._precompute(*args, **kwargs, device=x.device, dtype=x.dtype)
        return Delta._apply_precomputed(_p, x=x)

    @staticmethod
    def _check(seed) -> None:
        if not isinstance(seed, (tuple, list)):
            raise ValueError("seed must be tuple or list.")

    @staticmethod
    def _precompute(seed, static_out: bool, device: torch.device | None, dtype: torch.dtype | None) -> Precomputed:
        Delta._check(seed)
        return Precomputed(tensors={"window": to(tables.delta_window(seed, static_out), device=device, dtype=dtype)})

    @staticmethod
    def _forward(x: torch.Tensor, *, window: torch.Tensor) -> torch.Tensor:
        d = x.dim()
        if d == 2:
            x = x.unsqueeze(0)
        if x.dim() != 3:
            raise ValueError("Input must be 2D or 3D tensor.")
        y = ops.DeltaFn.apply(x, window)
        return y.squeeze(0) if d == 2 else y
