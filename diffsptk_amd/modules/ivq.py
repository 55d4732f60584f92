"""Inverse vector quantisation (reference: ivq.py): xq = codebook[indices], one launch of csrc/vq.hip.  The codebook is float32, as
VectorQuantization holds it; an index outside 0 .. K - 1 gives a row of NaN (the reference's index_select raises on the device).

The class is exported from the package root, not from diffsptk_amd.modules, for the reason given in modules/mlsacheck.py."""
from __future__ import annotations

import torch
from torch import nn

from .. import ops


class InverseVectorQuantization(nn.Module):
    def __init__(self):
        super().__init__()

    def forward(self, indices: torch.Tensor, codebook: torch.Tensor) -> torch.Tensor:
        """indices:(...) integers, codebook:(K, M+1) -> xq:(..., M+1) (ivq.py:63-67)."""
        return ops.vq_lookup(indices, codebook)
