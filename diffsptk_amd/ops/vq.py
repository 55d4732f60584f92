"""Vector quantisation and codebook design (csrc/vq.hip): the nearest-codeword search, the lookup, the quantiser with its straight-through
gradient, and one iteration of the Linde-Buzo-Gray algorithm on the device without a host read."""
from __future__ import annotations

import torch

from .. import _lib
from ._core import _call, _dtype_code, _p, _require_device, _stream


def _check_vq(x, codebook):
    """x:(T, L) float32 / float64 against codebook:(K, L) float32.  The ceiling first, the device last."""
    if codebook.dim() != 2 or codebook.size(0) < 1 or codebook.size(1) < 1:
        raise ValueError(f"vq: codebook must be (K, L), got {tuple(codebook.shape)}")
    L = codebook.size(1)
    if x.dim() != 2 or x.size(1) != L:
        raise ValueError(f"vq: x must be (T, {L}), got {tuple(x.shape)}")
    if L > _lib.VQ_MAX_LENGTH:
        raise ValueError(f"vq: vectors of {L} elements exceed DSA_VQ_MAX_LENGTH = {_lib.VQ_MAX_LENGTH}: the accumulation gives each column "
                         "a lane of one wave")
    _dtype_code(x)
    if codebook.dtype != torch.float32:
        raise RuntimeError(f"expected a float32 codebook but found {codebook.dtype}")
    _require_device(x, codebook)


def _partials(x):
    rows = _lib.VQ_TILE_BYTES // x.element_size()
    return torch.empty((x.size(0) + rows - 1) // rows, device=x.device, dtype=torch.float64)


def vq_search(x, codebook, return_xq=True, scale=None):
    """(indices:(T) int64, xq:(T, L) or None, partial, total): the first nearest codeword of every vector by float64 sums of squares;
    partial the per-workgroup sums of the minimal distances, total (0-d, x's dtype) scale times their sum, or None.  No host read."""
    _check_vq(x, codebook)
    xc, cb = x.contiguous(), codebook.contiguous()
    T, L = xc.shape
    indices = torch.empty(T, device=xc.device, dtype=torch.int64)
    xq = torch.empty_like(xc) if return_xq else None
    partial = _partials(xc)
    total = None if scale is None else torch.zeros((), device=xc.device, dtype=xc.dtype)
    with torch.cuda.device(xc.device):
        _call("dsa_vq_search", _p(xc), _p(cb), T, cb.size(0), L, _dtype_code(xc), _p(indices), _p(xq), _p(partial), _p(total),
              0.0 if scale is None else float(scale), _stream())
    return indices, xq, partial, total


def vq_lookup(indices, codebook, dtype=None):
    """codebook[indices]:(..., L) in dtype (default: the codebook's float32); an index outside the codebook gives NaN (ivq.py:63-67)."""
    if codebook.dim() != 2:
        raise ValueError(f"vq: codebook must be (K, L), got {tuple(codebook.shape)}")
    if codebook.dtype != torch.float32:
        raise RuntimeError(f"expected a float32 codebook but found {codebook.dtype}")
    _require_device(indices, codebook)
    idx, cb = indices.reshape(-1).long().contiguous(), codebook.contiguous()
    K, L = cb.shape
    xq = torch.empty(idx.numel(), L, device=cb.device, dtype=dtype or torch.float32)
    with torch.cuda.device(cb.device):
        _call("dsa_vq_lookup", _p(idx), _p(cb), idx.numel(), K, L, _dtype_code(xq), _p(xq), _stream())
    return xq.reshape(*indices.shape, L)


class _Quantize(torch.autograd.Function):
    """(xq, indices, loss) of x:(T, L): xq passes its cotangent straight through to x, loss = mean((x - xq)^2)."""

    @staticmethod
    def forward(ctx, x, codebook):
        indices, xq, _, loss = vq_search(x, codebook, True, 1.0 / max(x.numel(), 1))
        ctx.save_for_backward(x.contiguous(), xq)
        ctx.mark_non_differentiable(indices)
        return xq, indices, loss

    @staticmethod
    def backward(ctx, g_xq, _g_indices, g_loss):
        x, xq = ctx.saved_tensors
        g_xq = None if g_xq is None else g_xq.contiguous()
        g_loss = None if g_loss is None else g_loss.contiguous()
        gx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _call("dsa_vq_vjp", _p(g_xq), _p(g_loss), _p(x), _p(xq), x.numel(), _dtype_code(x), _p(gx), _stream())
        return gx, None


def vq_quantize(x, codebook):
    return _Quantize.apply(x, codebook)


def vq_accum_update(x, indices, partial, K, min_data, readback):
    """(pending:(K, L) float32, n_data:(K) int64) of lbg.py:264-285 from the assignment: two calls, no host read.  readback: a (3,)
    float64 device tensor that receives sum(partial) / T, the number of clusters below min_data and the first largest cluster."""
    T, L = x.shape
    dev = x.device
    pending = torch.empty(K, L, device=dev, dtype=torch.float32)
    n_data = torch.empty(K, device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        size = _lib.load().dsa_vq_accum_workspace_bytes(T, K, L)
        if size < 0:
            _lib.check(_lib.ERR_INVALID_ARGUMENT, "dsa_vq_accum_workspace_bytes")
        ws = torch.empty(size // 8, device=dev, dtype=torch.float64)
        _call("dsa_vq_accum", _p(x), _p(indices), T, K, L, _dtype_code(x), _p(ws), _stream())
        _call("dsa_vq_update", _p(ws), _p(partial), 0 if partial is None else partial.numel(), T, K, L, int(min_data), _p(n_data), _p(pending),
              _p(readback), _stream())
    return pending, n_data


def lbg_step(x, codebook, min_data, readback):
    """One iteration of lbg.py:252-285 on x:(T, L) contiguous and the live codebook:(K, L): E-step and M-step in three calls (four launches), the
    centroids into a pending buffer.  Returns (indices, pending, n_data).  No host read."""
    indices, _, partial, _ = vq_search(x, codebook, False)
    pending, n_data = vq_accum_update(x, indices, partial, codebook.size(0), min_data, readback)
    return indices, pending, n_data
