"""Dynamic time warping with a soft minimum (reference: dtw.py): the aligned distance of two vector sequences, differentiable in both,
and the Viterbi path.  The reference's T1 T2 Python iterations are one launch (csrc/dtw.hip), the gradient a second, the path a third.

Departures from the reference (include/diffsptk_amd.h, section a20):
  * a batch of more than one pair works, with per-pair `lengths` read on the device (the reference raises "Boolean value of Tensor with
    more than one value is ambiguous" there); a pair's result is, bit for bit, that of the pair run alone;
  * Manhattan, Euclidean and squared Euclidean distances are formed from differences for every size (cdist switches to the
    |x|^2 + |y|^2 - 2 x.y expansion beyond 25 rows);
  * `lengths` outside 1 .. T1, 1 .. T2 give a NaN distance, zero gradients and an empty path (the reference indexes from the end);
  * with return_indices=False nothing is read back to the host, so the call can be captured in a graph; return_indices=True reads the
    path lengths back once;
  * one pair's x and the resident diagonals must fit a compute unit's LDS: T1 (D + 12) elements in DSA_DTW_MAX_LDS_BYTES.

The class is exported from the package root and through functional.dtw / functional.dtw_merge, not from diffsptk_amd.modules, for the
reason given in modules/mlsacheck.py."""
from __future__ import annotations

import torch

from .. import _lib, ops
from ..utils.private import filter_values
from .base import BaseFunctionalModule, Precomputed

_METRICS = {0: _lib.DTW_MANHATTAN, "manhattan": _lib.DTW_MANHATTAN, 1: _lib.DTW_EUCLIDEAN, "euclidean": _lib.DTW_EUCLIDEAN,
            2: _lib.DTW_SQUARED_EUCLIDEAN, "squared-euclidean": _lib.DTW_SQUARED_EUCLIDEAN,
            3: _lib.DTW_SYMMETRIC_KL, "symmetric-kl": _lib.DTW_SYMMETRIC_KL}


class DynamicTimeWarping(BaseFunctionalModule):
    """x:(B, T1, D), (T1, D) or (T1,), y likewise with T2, lengths:(B, 2) or None -> distance:(B,), and with return_indices=True the list
    of the pairs' (T, 2) int64 Viterbi paths (dtw.py:161-209).  metric: "manhattan", "euclidean", "squared-euclidean", "symmetric-kl" or
    0 .. 3; p: the local path constraint, 0 .. 6; softness > 0: the smoothing of the minimum."""

    def __init__(self, metric: str | int = "euclidean", p: int = 4, softness: float = 1e-3) -> None:
        super().__init__()
        self._register_precomputed(self._precompute(**filter_values(locals())))

    def forward(self, x: torch.Tensor, y: torch.Tensor, lengths: torch.Tensor | None = None,
                return_indices: bool = False) -> torch.Tensor | tuple[torch.Tensor, list[torch.Tensor]]:
        return self._call_forward(x, y, lengths, return_indices)

    @staticmethod
    def _func(x: torch.Tensor, y: torch.Tensor, lengths: torch.Tensor | None, return_indices: bool, *args,
              **kwargs) -> torch.Tensor | tuple[torch.Tensor, list[torch.Tensor]]:
        pre = DynamicTimeWarping._precompute(*args, **kwargs)
        return DynamicTimeWarping._apply_precomputed(pre, x=x, y=y, lengths=lengths, return_indices=return_indices)

    @staticmethod
    def _check(softness: float) -> None:
        if softness <= 0:
            raise ValueError("softness must be positive.")

    @staticmethod
    def _precompute(metric: str | int, p: int, softness: float) -> Precomputed:
        DynamicTimeWarping._check(softness)
        if metric not in _METRICS:
            raise ValueError(f"metric {metric} is not supported.")
        if p not in range(7):
            raise ValueError(f"local path constraint type {p} is not supported.")
        return Precomputed(values={"metric": _METRICS[metric], "p": int(p), "softness": softness})

    @staticmethod
    def _forward(x: torch.Tensor, y: torch.Tensor, lengths: torch.Tensor | None, return_indices: bool, *, metric: int, p: int,
                 softness: float) -> torch.Tensor | tuple[torch.Tensor, list[torch.Tensor]]:
        if x.dim() == 1:   # the reference's reshapes and checks in the reference's order (dtw.py:313-330)
            x = x.reshape(1, -1, 1)
            y = y.reshape(1, -1, 1)
        elif x.dim() == 2:
            x = x.unsqueeze(0)
            y = y.unsqueeze(0)
        if x.dim() != 3:
            raise ValueError("x and y must be 1D, 2D, or 3D tensor.")
        if x.dim() != y.dim():
            raise ValueError("x and y must have the same number of dimensions.")
        if lengths is not None and lengths.dim() != 2:
            raise ValueError("lengths must be 2D tensor.")

        distance, R, R2 = ops.DtwFn.apply(x, y, lengths, metric, p, softness, return_indices)
        if not return_indices:
            return distance
        indices, count = ops.dtw_path(x, y, lengths, R, R2, metric, p)
        rows = indices.size(1)
        return distance, [indices[b, rows - n:] for b, n in enumerate(count.tolist())]   # the one host read of this module

    @staticmethod
    def merge(x: torch.Tensor, y: torch.Tensor, indices: torch.Tensor) -> torch.Tensor:
        """x:(T1, D) or (T1,), y:(T2, D) or (T2,), indices:(T, 2) -> (T, 2D) or (T, 2): the frames of both along the path (dtw.py:340-390)."""
        if x.dim() != y.dim():
            raise ValueError("x and y must have the same number of dimensions.")
        if indices.dim() != 2 or indices.size(-1) != 2:
            raise ValueError("The shape of indices must be (T, 2).")
        xs, ys = x[indices[:, 0]], y[indices[:, 1]]
        return torch.stack([xs, ys], dim=-1) if x.dim() == 1 else torch.cat([xs, ys], dim=-1)
