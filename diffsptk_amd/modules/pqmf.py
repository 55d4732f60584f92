"""Pseudo-QMF filter banks (reference: pqmf.py, ipqmf.py): subband analysis and synthesis, the front and back end of multi-band
vocoders.  Each runs as one launch forward and one backward (csrc/pqmf.hip); fuse(pqmf, Decimation) and fuse(Interpolation, ipqmf)
(modules/fused.py) fold the resampling into the same launches."""
from __future__ import annotations

import warnings

import numpy as np
import torch
from torch import nn

from .. import ops
from ..utils import tables
from ..utils.private import to


def _filters(n_band, filter_order, mode, alpha, kwargs, device, dtype) -> torch.Tensor:
    """(K, M+1), time-flipped as the reference stores them for conv1d (pqmf.py:200-208, ipqmf.py:79-87)."""
    filters, is_converged = tables.pqmf_filters(n_band, filter_order, mode=mode, alpha=alpha, **kwargs)
    if not is_converged:
        warnings.warn("Failed to find PQMF coefficients.")
    return to(np.flip(filters, 1).copy(), device=device, dtype=dtype)


class PseudoQuadratureMirrorFilterBankAnalysis(nn.Module):
    """x:(B, 1, T), (B, T) or (T,) -> y:(B, K, T): y[b,k,t] = sum_j h[k,j] xp[b, t + M - j], xp the signal after dl zeros and
    before dr copies of its last sample (pqmf.py:214-258).  `filters` is (K, 1, M+1), time-flipped, as in the reference: a
    Parameter with learnable=True, otherwise a non-persistent buffer."""

    def __init__(self, n_band: int, filter_order: int, alpha: float = 100, learnable: bool = False, device: torch.device | None = None,
                 dtype: torch.dtype | None = None, **kwargs) -> None:
        super().__init__()
        filters = _filters(n_band, filter_order, "analysis", alpha, kwargs, device, dtype).unsqueeze(1)
        if learnable:
            self.filters = nn.Parameter(filters)
        else:
            self.register_buffer("filters", filters, persistent=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._analyze(x, 1, 0)

    def _analyze(self, x: torch.Tensor, period: int, start: int) -> torch.Tensor:
        """pqmf.py:250-258, then x[..., start::period] of the result, in one launch."""
        if x.dim() == 1:
            x = x.view(1, 1, -1)
        elif x.dim() == 2:
            x = x.unsqueeze(1)
        if x.dim() != 3:
            raise ValueError("Input must be 1D tensor.")
        if x.size(1) != 1:
            raise RuntimeError(f"expected the input to have 1 channel, but got {x.size(1)} channels instead")
        return ops.PqmfFn.apply(x[:, 0], self.filters[:, 0], period, start)


class PseudoQuadratureMirrorFilterBankSynthesis(nn.Module):
    """y:(B, K, T) or (K, T) -> x:(B, 1, T), or (B, T) with keepdim=False: x[b,t] = sum_k sum_j g[k,j] yp[b, k, t + M - j]
    (ipqmf.py:93-141; for odd M the zero pad is the shorter one).  `filters` is (1, K, M+1), time-flipped, as in the reference."""

    def __init__(self, n_band: int, filter_order: int, alpha: float = 100, learnable: bool = False, device: torch.device | None = None,
                 dtype: torch.dtype | None = None, **kwargs) -> None:
        super().__init__()
        filters = _filters(n_band, filter_order, "synthesis", alpha, kwargs, device, dtype).unsqueeze(0)
        if learnable:
            self.filters = nn.Parameter(filters)
        else:
            self.register_buffer("filters", filters, persistent=False)

    def forward(self, y: torch.Tensor, keepdim: bool = True) -> torch.Tensor:
        return self._synthesize(y, 1, 0, keepdim)

    def _synthesize(self, y: torch.Tensor, up: int, start: int, keepdim: bool) -> torch.Tensor:
        """ipqmf.py:132-141 on the Interpolation(up, start) of y, in one launch."""
        if y.dim() == 2:
            y = y.unsqueeze(0)
        if y.dim() != 3:
            raise ValueError("Input must be 3D tensor.")
        if y.size(1) != self.filters.size(1):
            raise RuntimeError(f"expected the input to have {self.filters.size(1)} channels, but got {y.size(1)} channels instead")
        x = ops.IpqmfFn.apply(y, self.filters[0], up, start)
        return x.unsqueeze(1) if keepdim else x
