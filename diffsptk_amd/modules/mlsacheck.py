"""Stability check of the MLSA digital filter (reference: mlsacheck.py): the mel-cepstrum scaled or clipped where the amplitude of
its gain-free part passes the threshold of the filter's Pade approximation -- one launch forward and one backward (csrc/mlsacheck.hip).

Two departures from the reference (include/diffsptk_amd.h, section a16):
  * in fast mode and with an even n_fft, a frame that is not modified is returned with the input's bits and its gradient is the
    cotangent's bits (the reference re-rounds it through (c0 - gain) * 1 + gain and its FFT pair); with an odd n_fft the reference's
    irfft has another length than its rfft and changes every frame: so it does here;
  * an n_fft with 2 * (n_fft // 2) < cep_order + 1 raises ValueError at _precompute (the reference returns a tensor of the wrong width).

The class is exported from the package root and through functional.mlsacheck, not yet from diffsptk_amd.modules: the alignment sweep's
table (tests/alignment_rows.py) has a row per name of modules.__all__, and its row arrives with the change that may edit that table."""
from __future__ import annotations

import warnings

import torch

from .. import ops
from ..utils.private import check_size, filter_values
from .base import BaseFunctionalModule, Precomputed


class MLSADigitalFilterStabilityCheck(BaseFunctionalModule):
    """mc:(..., M+1) -> the mel-cepstrum whose MLSA filter stays within the range of its Pade approximation (mlsacheck.py:181-230):
    scaled as a whole (mod_type "scale"; fast: by the plain sum, else by the largest amplitude over n_fft // 2 + 1 bins) or clipped bin
    by bin ("clip").  warn_type "ignore" never synchronises (it runs under graph capture); "warn" and "exit" read one flag back from
    the device, as the reference's torch.any does."""

    _takes_input_size = True

    def __init__(
        self,
        cep_order: int,
        *,
        alpha: float = 0,
        pade_order: int = 4,
        strict: bool = True,
        threshold: float | None = None,
        fast: bool = True,
        n_fft: int = 256,
        warn_type: str = "warn",
        mod_type: str = "scale",
        device: torch.device | None = None,
        dtype: torch.dtype | None = None,
    ) -> None:
        super().__init__()
        self.in_dim = cep_order + 1
        self._register_precomputed(self._precompute(**filter_values(locals())))

    def forward(self, mc: torch.Tensor) -> torch.Tensor:
        check_size(mc.size(-1), self.in_dim, "dimension of mel-cepstrum")
        return self._call_forward(mc)

    @staticmethod
    def _func(mc: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        pre = MLSADigitalFilterStabilityCheck._precompute(mc.size(-1) - 1, *args, **kwargs, device=mc.device, dtype=mc.dtype)
        return MLSADigitalFilterStabilityCheck._apply_precomputed(pre, mc=mc)

    @staticmethod
    def _check(cep_order: int) -> None:
        if cep_order < 0:
            raise ValueError("cep_order must be non-negative.")

    @staticmethod
    def _precompute(cep_order: int, alpha: float, pade_order: int, strict: bool, threshold: float | None, fast: bool, n_fft: int,
                    warn_type: str, mod_type: str, device: torch.device | None = None, dtype: torch.dtype | None = None) -> Precomputed:
        MLSADigitalFilterStabilityCheck._check(cep_order)
        if threshold is None:   # mlsacheck.py:153-163
            table = {4: (4.5, 6.20), 5: (6.0, 7.65), 6: (7.4, 9.13), 7: (8.9, 10.6)}
            if pade_order not in table:
                raise ValueError(f"pade_order {pade_order} is not supported.")
            threshold = table[pade_order][0 if strict else 1]
        if not fast and 2 * (n_fft // 2) < cep_order + 1:   # a departure: the reference returns 2 * (n_fft // 2) columns
            raise ValueError(f"n_fft {n_fft} is too short for cep_order {cep_order}: 2 * (n_fft // 2) must be at least cep_order + 1.")
        return Precomputed(values={"alpha": alpha, "threshold": threshold, "fast": fast, "n_fft": n_fft, "warn_type": warn_type,
                                   "mod_type": mod_type})

    @staticmethod
    def _forward(mc: torch.Tensor, *, alpha: float, threshold: float, fast: bool, n_fft: int, warn_type: str, mod_type: str) -> torch.Tensor:
        if mod_type not in ("clip", "scale"):
            raise ValueError(f"mod_type {mod_type} is not supported.")
        if fast and mod_type == "clip":
            raise ValueError("clip is not supported in fast mode.")
        out, unstable = ops.mlsacheck(mc, alpha, threshold, "fast" if fast else mod_type, n_fft, detect=warn_type != "ignore")
        if unstable is not None and unstable.item():
            if warn_type == "warn":
                warnings.warn("Detected unstable MLSA filter.")
            elif warn_type == "exit":
                raise RuntimeError("Detected unstable MLSA filter.")
            else:
                raise ValueError(f"warn_type {warn_type} is not supported.")
        return out
