"""Vector quantisation (reference: vq.py): the nearest codeword of a (K, M+1) float32 codebook for every (M+1)-vector, by one launch of
csrc/vq.hip whose sums of squares are float64 whatever the input's type.

What differs from the reference (include/diffsptk_amd.h, section a23):
  * the reference hands everything to the package `vector_quantize_pytorch`; this module does not use it and claims no parity with it.
    `codebook` is a float32 (K, M+1) buffer of the module itself (state_dict key "codebook"), initialised with torch.randn;
  * the nearest codeword is found from float64 sums of (x - c)^2 formed from the values as stored, for float32 and float64 input alike;
    on a tie the first index wins;
  * eval mode: (xq, indices, loss) with loss = 0 and no graph;
  * training mode: xq carries the straight-through gradient to x, and loss = mean((x - xq)^2), the commitment loss of van den Oord
    et al. with weight 1, differentiable in x (one backward launch for both cotangents).  The codebook is NOT updated: there is no
    exponential moving average and no codebook loss.  Design a codebook with LindeBuzoGrayAlgorithm;
  * `**kwargs` of the constructor and of `forward` are the package's options in the reference; here any of them raises TypeError;
  * M + 1 <= DSA_VQ_MAX_LENGTH (64).

The class is exported from the package root, not from diffsptk_amd.modules, for the reason given in modules/mlsacheck.py."""
from __future__ import annotations

import torch
from torch import nn

from .. import ops


def _no_kwargs(where: str, kwargs) -> None:
    if kwargs:
        raise TypeError(f"{where} got the keyword argument '{next(iter(kwargs))}': the reference passes it to the package "
                        "vector_quantize_pytorch, which diffsptk_amd does not use")


class VectorQuantization(nn.Module):
    """order M >= 0, codebook_size K >= 1 (vq.py:47-65)."""

    def __init__(self, order: int, codebook_size: int, device: torch.device | None = None, **kwargs) -> None:
        super().__init__()

        if order < 0:
            raise ValueError("order must be non-negative.")
        if codebook_size <= 0:
            raise ValueError("codebook_size must be positive.")
        _no_kwargs("VectorQuantization", kwargs)

        self.order = order
        self.codebook_size = codebook_size
        self.register_buffer("codebook", torch.randn(codebook_size, order + 1, device=device, dtype=torch.float32))

    def forward(self, x: torch.Tensor, codebook: torch.Tensor | None = None, **kwargs):
        """x:(..., M+1) -> (xq:(..., M+1) in x's dtype, indices:(...) int64, loss: 0-d).  codebook:(K, M+1), when given, is copied into
        the module's buffer first, as the reference does (vq.py:110-125)."""
        _no_kwargs("VectorQuantization.forward", kwargs)
        if codebook is not None:
            with torch.no_grad():
                self.codebook[:] = codebook.view_as(self.codebook)
        L = self.order + 1
        if x.size(-1) != L:
            raise ValueError(f"dimension of x must be {L}, got {x.size(-1)}.")
        x2 = x.reshape(-1, L)
        if self.training:
            xq, indices, loss = ops.vq_quantize(x2, self.codebook)
        else:
            with torch.no_grad():
                indices, xq, _, _ = ops.vq_search(x2, self.codebook)
                loss = torch.zeros((), device=x.device, dtype=x.dtype)
        return xq.reshape(x.shape), indices.reshape(x.shape[:-1]), loss
