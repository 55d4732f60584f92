"""Maximum likelihood parameter generation (reference: mlpg.py) as a banded Cholesky solve (csrc/paramgen.hip).

Departures from the reference (include/diffsptk_amd.h, section a19):
  * the module keeps the (H, L) window, the (H) thresholds and the (T, L) banded Cholesky factor of W^T W, not the dense (T, T H)
    matrix M = (W^T W)^-1 W^T of mlpg.py:159-163: neither W nor M is ever formed;
  * a sequence shorter than 2N = L - 1 frames raises ValueError at _precompute: the reference cannot build its matrix there and fails
    with a shape-mismatch RuntimeError (mlpg.py:152);
  * functional.mlpg caches the factor per (T, seed, device, dtype); the reference rebuilds its matrix on every call.

The class is exported from the package root and through functional.mlpg, not yet from diffsptk_amd.modules (modules/delta.py)."""
from __future__ import annotations

import functools

import torch

from .. import ops
from ..utils import tables
from ..utils.private import check_size, filter_values, to
from .base import BaseFunctionalModule, Precomputed


def _freeze(seed):
    return tuple(_freeze(s) for s in seed) if isinstance(seed, (tuple, list)) else seed


def _thaw(seed):
    return [_thaw(s) for s in seed] if isinstance(seed, tuple) else seed


@functools.lru_cache(maxsize=32)
def _tensors(size: int, seed, device, dtype):
    seed = _thaw(seed)
    window = tables.delta_window(seed, True)
    th = tables.mlpg_threshold(seed)
    N = (window.shape[1] - 1) // 2
    if size < 2 * N:
        raise ValueError(f"size must be at least {2 * N} for windows of length {window.shape[1]}.")
    factor = tables.mlpg_factor(size, window, th)
    return {"window": to(window, device=device, dtype=dtype), "th": torch.from_numpy(th).to(device), "factor": to(factor, device=device, dtype=dtype)}


class MaximumLikelihoodParameterGeneration(BaseFunctionalModule):
    """u:(..., T, D H), as Delta writes it -> (..., T, D): the static trajectory that is most likely under unit variances given the
    static and dynamic means (mlpg.py:165-171).  size: the sequence length T; seed: as for Delta."""

    _takes_input_size = True

    def __init__(
        self,
        size: int,
        seed=[[-0.5, 0, 0.5], [1, -2, 1]],
        device: torch.device | None = None,
        dtype: torch.dtype | None = None,
    ) -> None:
        super().__init__()
        self.in_length = size
        self._register_precomputed(self._precompute(**filter_values(locals())))

    def forward(self, u: torch.Tensor) -> torch.Tensor:
        check_size(u.size(-2), self.in_length, "length of input")
        return self._call_forward(u)

    @staticmethod
    def _func(u: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        _p = MaximumLikelihoodParameterGeneration._precompute(u.size(-2), *args, **kwargs, device=u.device, dtype=u.dtype, cache=True)
        return MaximumLikelihoodParameterGeneration._apply_precomputed(_p, mean=u)

    @staticmethod
    def _check() -> None:
        pass

    @staticmethod
    def _precompute(size: int, seed, device: torch.device | None, dtype: torch.dtype | None, cache: bool = False) -> Precomputed:
        MaximumLikelihoodParameterGeneration._check()
        if not isinstance(seed, (tuple, list)):
            raise ValueError("seed must be tuple or list.")
        key = (int(size), _freeze(seed), None if device is None else torch.device(device), dtype or torch.get_default_dtype())
        build = _tensors if cache else _tensors.__wrapped__   # (a module owns its tensors; the functional form shares them)
        return Precomputed(tensors=build(*key))

    @staticmethod
    def _forward(mean: torch.Tensor, *, window: torch.Tensor, th: torch.Tensor, factor: torch.Tensor) -> torch.Tensor:
        return ops.MlpgFn.apply(mean, window, th, factor)
