"""Mel-cepstrum postfiltering (reference: mcpf.py) in closed form, one launch forward and one backward (csrc/paramgen.hip).

The reference chains freqt -> rfft -> exp -> hfft twice, then mc2b and b2mc.  b2mc(mc2b(.)) is the identity and b[0] enters only mc[0],
so the operator is out = w * mc with out[0] += log(e1 / e2) / 2, e the energy of the impulse response: the sum of exp(2 Re C_k) over the
ir_length-point spectrum of the de-warped cepstrum (include/diffsptk_amd.h, section a19).

Departures from the reference:
  * the module keeps the (bins, M + 1) float64 table of utils.tables.mcpf_table and its transpose, for either dtype, and no sub-module
    and no weight tensor: the weight 1 + beta is a scalar;
  * ir_length must lie in 2 .. 4096 (ValueError): the reference fails inside hfft at 1 and has no upper bound;
  * every sum is float64; for an odd ir_length the reference's hfft has ir_length - 1 points, and so it is here.

The class is exported from the package root and through functional.mcpf, not yet from diffsptk_amd.modules (modules/delta.py)."""
from __future__ import annotations

import torch

from .. import _lib, ops
from ..utils import tables
from ..utils.private import check_size, filter_values, to
from .base import BaseFunctionalModule, Precomputed


class MelCepstrumPostfiltering(BaseFunctionalModule):
    """mc:(..., M+1) -> the mel-cepstrum with its formants emphasised: the coefficients from `onset` on scaled by 1 + beta and the
    energy of the impulse response (ir_length samples) kept (mcpf.py:191-209)."""

    _takes_input_size = True

    def __init__(
        self,
        cep_order: int,
        alpha: float = 0,
        beta: float = 0,
        onset: int = 2,
        ir_length: int = 128,
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
        _p = MelCepstrumPostfiltering._precompute(mc.size(-1) - 1, *args, **kwargs, device=mc.device, dtype=mc.dtype, module=False)
        return MelCepstrumPostfiltering._apply_precomputed(_p, mc=mc)

    @staticmethod
    def _check(onset: int) -> None:
        if onset < 0:
            raise ValueError("onset must be non-negative.")

    @staticmethod
    def _precompute(cep_order: int, alpha: float, beta: float, onset: int, ir_length: int, device: torch.device | None,
                    dtype: torch.dtype | None, module: bool = True) -> Precomputed:
        MelCepstrumPostfiltering._check(onset)
        if cep_order < 0:
            raise ValueError("cep_order must be non-negative.")
        if abs(alpha) >= 1:
            raise ValueError("alpha must be in (-1, 1).")
        if not 2 <= ir_length <= 2 * (_lib.MCPF_MAX_BINS - 1):
            raise ValueError(f"ir_length must be in 2 .. {2 * (_lib.MCPF_MAX_BINS - 1)}.")
        table = tables.mcpf_table(cep_order, alpha, ir_length)
        return Precomputed(values={"scale": 1 + beta, "onset": onset},
                           tensors={"table": to(table, device=device, dtype=torch.float64),
                                    "table_t": to(table.T, device=device, dtype=torch.float64)})

    @staticmethod
    def _forward(mc: torch.Tensor, *, scale: float, onset: int, table: torch.Tensor, table_t: torch.Tensor) -> torch.Tensor:
        return ops.McpfFn.apply(mc, table, table_t, scale, onset)
