"""Signal generators with the reference's signatures (signals.py): the Gaussian and M-sequence noises that stand beside the excitation.
Host arithmetic and stock torch generators: nothing here is a hot path."""
from __future__ import annotations

import math

import numpy as np
import torch


def _shape(order) -> list[int]:
    # signals.py:271-275: `order` is the LAST INDEX of the last dimension
    shape = list(order[0]) if len(order) == 1 and isinstance(order[0], (list, tuple)) else list(order)
    shape[-1] += 1
    return shape


def _mseq_bits(length: int) -> np.ndarray:
    """The first `length` outputs of the 32-bit shift register of signals.py:280-299 as 0 / 1.

    With s the register's bit stream (s_k = bit k of 0x55555555 for k < 32) every pass shifts once, emits the new bit 0 and sets bit 31
    to bit 0 xor bit 28: s_m = s_{m-31} ^ s_{m-3}, and output i is s_{i+1}.  Over GF(2) the recurrence also holds with both lags
    multiplied by any power of two (its characteristic polynomial squares to itself in x^2), so a stream of which L >= 31 * 2^k bits are
    known grows by 3 * 2^k bits in one vector operation."""
    s = np.zeros(max(length + 1, 32), dtype=np.uint8)
    s[:32] = [(0x55555555 >> k) & 1 for k in range(32)]
    known = 32
    while known < length + 1:
        k = 1 << max(0, int(math.floor(math.log2(known / 31))))
        while 31 * k > known:
            k >>= 1
        n = min(3 * k, length + 1 - known)
        s[known:known + n] = s[known - 31 * k:known - 31 * k + n] ^ s[known - 3 * k:known - 3 * k + n]
        known += n
    return s[1:length + 1]


def mseq(*order: int, **kwargs) -> torch.Tensor:
    """M-sequence of +-1 (signals.py:244-301): mseq(M) has M + 1 values, mseq(A, M) the shape (A, M + 1) filled in flattened order.
    **kwargs as torch.ones.  The register runs on the host."""
    shape = _shape(order)
    like = torch.ones(0, **kwargs)
    bits = _mseq_bits(math.prod(shape))
    out = torch.from_numpy(bits.astype(np.float64) * 2.0 - 1.0).to(device=like.device, dtype=like.dtype)
    return out.reshape(shape)


def mseq_like(tensor: torch.Tensor, **kwargs) -> torch.Tensor:
    """M-sequence with the shape, device and dtype of `tensor` (signals.py:304-331)."""
    shape = list(tensor.shape)
    shape[-1] -= 1
    return mseq(*shape, device=tensor.device, dtype=tensor.dtype, **kwargs)


def nrand(*order: int, mean: float = 0, stdv: float = 1, var: float | None = None, **kwargs) -> torch.Tensor:
    """Gaussian noise (signals.py:334-387): nrand(M) has M + 1 values.  **kwargs as torch.randn."""
    if var is not None:
        stdv = var**0.5
    if stdv < 0:
        raise ValueError("stdv must be non-negative.")
    x = torch.randn(*_shape(order), **kwargs)
    return x * stdv + mean
