"""Yingram (reference: yingram.py): the pitch feature of YIN -- the cumulative-mean-normalised difference function of a frame, read on a
semitone grid of lags by linear interpolation.  One launch forward and one backward (csrc/yingram.hip), with the lag sums either as
they are written or through the LDS transform; ``fuse(frame, yingram)`` reads the waveform itself.

Two departures from the reference (include/diffsptk_amd.h, section a22):
  * option sets whose largest lag lies in (lag_max - 1, lag_max] -- frame_length=32, sample_rate=8000, lag_min=1 with the default
    lag_max, or lag_min=2, lag_max=29 -- raise ValueError at _precompute, naming the lag and lag_max.  The reference builds the module
    and raises IndexError in forward: its lags_ceil points one past the lag_max - 1 values of the difference function;
  * a lag that is an integer (lags_ceil == lags_floor; it takes a sample_rate that is a multiple of 440, 8800 for instance) returns
    d'[lag], the limit of the interpolation, and its gradient goes to d'[lag].  The reference divides 0 by 0 there and returns NaN.

``algo`` (an attribute, ops._lib.ALGO_AUTO by default) pins the route: ALGO_GENERIC the direct lag sums, ALGO_TUNED the transform.

The class is exported from the package root and through functional.yingram, not from diffsptk_amd.modules, for the reason given in
modules/mlsacheck.py."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib, ops
from ..utils.private import check_size, filter_values, to
from .base import BaseFunctionalModule, Precomputed
from .spec import device_twiddle


_FUNCTIONAL_TABLES: dict = {}


class Yingram(BaseFunctionalModule):
    """x:(..., L) framed waveform -> (..., M) Yingram (yingram.py:81-106), M bins of 1 / n_bin semitone between the MIDI notes of
    lag_max and lag_min.  sample_rate >= 8000; 1 <= lag_min <= lag_max < L, lag_max = L - 1 when None; n_bin >= 1."""

    _takes_input_size = True

    def __init__(
        self,
        frame_length: int,
        sample_rate: int = 22050,
        lag_min: int = 22,
        lag_max: int | None = None,
        n_bin: int = 20,
        device: torch.device | None = None,
        dtype: torch.dtype | None = None,
    ) -> None:
        super().__init__()
        self.in_dim = frame_length
        self._register_precomputed(self._precompute(**filter_values(locals())))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        check_size(x.size(-1), self.in_dim, "frame length")
        return self._call_forward(x)

    @staticmethod
    def _func(x: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        key = (x.size(-1), args, tuple(sorted(kwargs.items())), str(x.device), x.dtype)   # the tables of the functional path, kept per option set
        pre = _FUNCTIONAL_TABLES.get(key)
        if pre is None:
            pre = _FUNCTIONAL_TABLES[key] = Yingram._precompute(x.size(-1), *args, **kwargs, device=x.device, dtype=x.dtype)
        return Yingram._apply_precomputed(pre, x=x)

    @staticmethod
    def _check(frame_length: int, sample_rate: int, lag_min: int, lag_max: int, n_bin: int) -> None:
        if sample_rate < 8000:
            raise ValueError("sample_rate must be greater than or equal to 8000.")
        if not (1 <= lag_min <= lag_max < frame_length):
            raise ValueError("Invalid lag_min and lag_max.")
        if n_bin <= 0:
            raise ValueError("n_bin must be positive.")

    @staticmethod
    def _precompute(frame_length: int, sample_rate: int, lag_min: int, lag_max: int | None, n_bin: int,
                    device: torch.device | None, dtype: torch.dtype | None) -> Precomputed:
        if lag_max is None:
            lag_max = frame_length - 1
        Yingram._check(frame_length, sample_rate, lag_min, lag_max, n_bin)
        # yingram.py:140-156: MIDI notes from the one of lag_max up to the one of lag_min, n_bin steps per semitone, as lags in float64
        midi_min = int(np.ceil(12 * np.log2(sample_rate / (440 * lag_max)) + 69))
        midi_max = int(12 * np.log2(sample_rate / (440 * lag_min)) + 69)
        # (built on the host and moved: the check below reads the tables, and a read of device tensors would synchronise every call of
        #  functional.yingram with the device)
        midi = torch.arange(midi_min, midi_max + 1, 1 / n_bin, dtype=torch.double)
        lags = sample_rate / (440 * 2 ** ((midi - 69) / 12))
        lags_ceil = lags.ceil().long()
        lags_floor = lags.floor().long()
        if lags.numel() and int(lags_ceil.max()) > lag_max - 1:
            raise ValueError(f"The largest lag, {float(lags.max()):.6g}, needs the difference function at {int(lags_ceil.max())}, beyond "
                             f"lag_max - 1 = {lag_max - 1}: lower lag_max = {lag_max} to a value the MIDI grid's largest lag stays below.")
        ramp = torch.arange(1, lag_max)
        return Precomputed(values={"algo": _lib.ALGO_AUTO},
                           tensors={"lags": to(lags, device=device, dtype=dtype), "lags_ceil": lags_ceil.to(device),
                                    "lags_floor": lags_floor.to(device), "ramp": ramp.to(device)})

    @staticmethod
    def _forward(x: torch.Tensor, *, lags: torch.Tensor, lags_ceil: torch.Tensor, lags_floor: torch.Tensor, ramp: torch.Tensor,
                 algo: int = _lib.ALGO_AUTO) -> torch.Tensor:
        lag_max = len(ramp) + 1
        twiddle = device_twiddle(ops.yingram_fft_length(x.size(-1), lag_max), x.device, x.dtype)
        return ops.YingramFn.apply(x, lags, lags_floor, lags_ceil, twiddle, lag_max, algo)
