"""Perceptual linear prediction of power spectra (reference: plp.py) -- the front-end feature that joins the filter-bank and LPC
branches."""
from __future__ import annotations

import torch

from .. import ops
from ..utils import tables
from ..utils.private import check_size, filter_values, to
from . import _learnable
from .base import BaseFunctionalModule, Precomputed
from .fbank import MelFilterBankAnalysis
from .levdur import LevinsonDurbin
from .mgc2mgc import MelGeneralizedCepstrumToMelGeneralizedCepstrum

_FORMATS = {0: "y", "y": "y", 1: "yE", "yE": "yE", 2: "yc", "yc": "yc", 3: "ycE", "ycE": "ycE"}


class PerceptualLinearPredictiveCoefficientsAnalysis(BaseFunctionalModule):
    """x:(..., L/2+1) power spectrum -> PLP (..., M) (+ C0 / energy), plp.py:312-320: power-domain filter bank, then equal
    loudness, compression, replicate1, hfft, Levinson-Durbin (eps = 0), the n_fft-point LPC -> cepstrum conversion of mgc2mgc,
    lifter and formatter.  The filter bank is dsa_fbank_fwd; everything after it is ONE launch (dsa_plp_fwd, csrc/plp.hip), whose
    constants are one packed table (tables.plp_table, float64 then cast)."""

    _takes_input_size = True

    # plp.py:247-265: the reference keeps the learnable filter bank in its fbank layer
    _reference_state_keys = {"H": ("fbank.H", None)}

    def __init__(self, *, fft_length: int, plp_order: int, n_channel: int, sample_rate: int, compression_factor: float = 0.33,
                 lifter: int = 1, f_min: float = 0, f_max: float | None = None, floor: float = 1e-5, gamma: float = 0,
                 scale: str = "htk", erb_factor: float | None = None, n_fft: int = 512, out_format: str | int = "y",
                 learnable: bool = False, device=None, dtype=None) -> None:
        super().__init__()
        self.in_dim = fft_length // 2 + 1
        # learnable: the filter bank H becomes a Parameter (the tail's table stays fixed)
        self._register_precomputed(self._precompute(**filter_values(locals(), drop_keys=["learnable"])),
                                   ("H",) if learnable else False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        check_size(x.size(-1), self.in_dim, "dimension of spectrum")
        return self._call_forward(x)

    @staticmethod
    def _func(x: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        pre = PerceptualLinearPredictiveCoefficientsAnalysis._precompute(2 * x.size(-1) - 2, *args, **kwargs, device=x.device,
                                                                         dtype=x.dtype)
        return PerceptualLinearPredictiveCoefficientsAnalysis._apply_precomputed(pre, x=x)

    @staticmethod
    def _check(plp_order: int, n_channel: int, compression_factor: float, lifter: int) -> None:
        if plp_order < 0:
            raise ValueError("plp_order must be non-negative.")
        if n_channel <= plp_order:
            raise ValueError("plp_order must be less than n_channel.")
        if compression_factor <= 0:
            raise ValueError("compression_factor must be positive.")
        if lifter < 0:
            raise ValueError("lifter must be non-negative.")

    @staticmethod
    def _precompute(fft_length, plp_order, n_channel, sample_rate, compression_factor=0.33, lifter=1, f_min=0, f_max=None,
                    floor=1e-5, gamma=0, scale="htk", erb_factor=None, n_fft=512, out_format="y", device=None,
                    dtype=None) -> Precomputed:
        # the reference's order (plp.py:213-305): PLP's checks, out_format, the filter bank, levdur, lpc2c (n_fft), the tables
        PerceptualLinearPredictiveCoefficientsAnalysis._check(plp_order, n_channel, compression_factor, lifter)
        if out_format not in _FORMATS:
            raise ValueError(f"out_format {out_format} is not supported.")
        MelFilterBankAnalysis._check(fft_length, n_channel, sample_rate, f_min, f_max, floor, gamma, erb_factor)
        H = tables.fbank_matrix(fft_length, n_channel, sample_rate, f_min, f_max, scale, erb_factor)
        LevinsonDurbin._check(plp_order, 0)
        MelGeneralizedCepstrumToMelGeneralizedCepstrum._check(plp_order, plp_order, 0, 0, -1, 0, True, n_fft)
        if plp_order > ops._lib.PLP_MAX_ORDER:
            raise ValueError(f"plp_order above {ops._lib.PLP_MAX_ORDER} is not supported by the kernels.")
        table = tables.plp_table(n_channel, plp_order, n_fft, sample_rate, f_min, f_max, scale, lifter)
        return Precomputed(values={"floor": floor, "gamma": gamma, "compression_factor": compression_factor,
                                   "plp_order": plp_order, "n_fft": n_fft, "out_format": _FORMATS[out_format]},
                           tensors={"H": to(H, device=device, dtype=dtype), "table": to(table, device=device, dtype=dtype)})

    @staticmethod
    def _forward(x: torch.Tensor, *, floor: float, gamma: float, compression_factor: float, plp_order: int, n_fft: int,
                 out_format: str, H: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
        if H.requires_grad:
            y, E = _learnable.fbank_with_weights(x, H, floor, gamma, True)
        else:
            y, E = ops.FbankFn.apply(x, H, floor, gamma, True)   # plp.py:248: use_power=True
        return ops.PlpFn.apply(y, E if "E" in out_format else None, table, plp_order, n_fft, compression_factor, out_format)
