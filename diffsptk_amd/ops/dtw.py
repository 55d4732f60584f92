"""Dynamic time warping with a soft minimum (csrc/dtw.hip): the aligned distance, its gradient, the Viterbi path."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ._core import _call, _dtype_code, _p, _require_device, _same_dtype, _stream

DTW_TWO_TABLES = (4, 6)   # the local path constraints whose axis steps read a second table (dtw.py:272-283)


def _check_dtw(x, y, lengths):
    if x.dim() != 3 or y.dim() != 3 or x.size(0) != y.size(0):
        raise ValueError(f"dtw: x and y must be (B, T1, D) and (B, T2, D), got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.size(2) != y.size(2):   # (the text of the reference's cdist)
        raise RuntimeError(f"X1 and X2 must have the same number of columns. X1: {x.size(2)} X2: {y.size(2)}")
    if x.size(1) == 0 or y.size(1) == 0:
        raise ValueError("dtw: x and y must not be empty sequences")
    if lengths is not None and (lengths.dim() != 2 or tuple(lengths.shape) != (x.size(0), 2) or lengths.dtype.is_floating_point):
        raise ValueError(f"dtw: lengths must be a (B, 2) integer tensor, got {tuple(lengths.shape)} of {lengths.dtype}")
    need = x.size(1) * (x.size(2) + 12) * x.element_size()
    if need > _lib.DTW_MAX_LDS_BYTES:
        raise ValueError(f"dtw: T1 (D + 12) elements take {need} bytes: x and the resident diagonals of one pair must fit "
                         f"DSA_DTW_MAX_LDS_BYTES = {_lib.DTW_MAX_LDS_BYTES} bytes of LDS")
    _same_dtype(x, y)
    _dtype_code(x)
    _require_device(x, y, lengths)


class DtwFn(torch.autograd.Function):
    """x:(B, T1, D), y:(B, T2, D), lengths:(B, 2) integer or None -> (distance:(B), R, R2).  R and R2 are the recursion's tables (T1 T2
    values per pair, laid out by anti-diagonal; R2 only for p = 4, 6), kept when an input needs a gradient or `tables` is set (for
    dtw_path), else None.  Saved for the backward: x, y, lengths and the tables.  No host read."""

    @staticmethod
    def forward(ctx, x, y, lengths, metric, p, softness, tables):
        _check_dtw(x, y, lengths)
        xc, yc = x.contiguous(), y.contiguous()
        lc = None if lengths is None else lengths.to(torch.int64).contiguous()
        B, T1, D = xc.shape
        T2 = yc.size(1)
        keep = bool(tables) or any(ctx.needs_input_grad[:2])
        dist = torch.empty(B, device=xc.device, dtype=xc.dtype)
        R = torch.empty(B, T1 * T2, device=xc.device, dtype=xc.dtype) if keep else None
        R2 = torch.empty_like(R) if keep and p in DTW_TWO_TABLES else None
        if B:
            with torch.cuda.device(xc.device):
                _call("dsa_dtw", _p(xc), _p(yc), _p(lc), B, T1, T2, D, metric, p, float(softness), _dtype_code(xc), _p(R), _p(R2), _p(dist), _stream())
        ctx.cfg = (metric, p, float(softness))
        ctx.lengths = lc
        ctx.save_for_backward(xc, yc, R, R2)
        ctx.mark_non_differentiable(*(t for t in (R, R2) if t is not None))
        return dist, R, R2

    @staticmethod
    @once_differentiable
    def backward(ctx, gdist, _gR, _gR2):
        xc, yc, R, R2 = ctx.saved_tensors
        metric, p, softness = ctx.cfg
        B, T1, D = xc.shape
        gx, gy = torch.empty_like(xc), torch.empty_like(yc)
        if B:
            gc = gdist.contiguous()
            with torch.cuda.device(xc.device):
                _call("dsa_dtw_vjp", _p(xc), _p(yc), _p(ctx.lengths), _p(R), _p(R2), _p(gc), B, T1, yc.size(1), D, metric, p, softness, _dtype_code(xc),
                      _p(gx), _p(gy), _stream())
        return gx, gy, None, None, None, None, None


def dtw_path(x, y, lengths, R, R2, metric, p):
    """(indices:(B, T1 + T2 - 1, 2) int64, count:(B) int32) from the tables of DtwFn: pair b's Viterbi path is
    indices[b, T1 + T2 - 1 - count[b]:].  No host read here; the caller reads `count` to cut the rows."""
    _check_dtw(x, y, lengths)
    xc, yc = x.detach().contiguous(), y.detach().contiguous()
    lc = None if lengths is None else lengths.to(torch.int64).contiguous()
    B, T1, D = xc.shape
    T2 = yc.size(1)
    indices = torch.empty(B, T1 + T2 - 1, 2, device=xc.device, dtype=torch.int64)
    count = torch.empty(B, device=xc.device, dtype=torch.int32)
    if B:
        with torch.cuda.device(xc.device):
            _call("dsa_dtw_path", _p(xc), _p(yc), _p(lc), _p(R), _p(R2), B, T1, T2, D, metric, p, _dtype_code(xc), _p(indices), _p(count), _stream())
    return indices, count
