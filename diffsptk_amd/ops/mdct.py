"""Lapped transforms (csrc/mdct.hip): MDCT / MDST and their inverses, each the other's adjoint."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ._core import _call, _dtype_code, _p, _require_device, _same_dtype, _stream

MDCT_TRANSFORMS = {"cosine": _lib.MDCT_COSINE, "sine": _lib.MDCT_SINE}


def mdct_fast_supported(frame_length: int, dtype) -> bool:
    """Whether dsa_mdct_analysis / dsa_mdct_synthesis run their fast kernels: float32 and a power-of-two frame length in range."""
    L = int(frame_length)
    return dtype == torch.float32 and L & (L - 1) == 0 and _lib.MDCT_FAST_MIN_LENGTH <= L <= _lib.MDCT_FAST_MAX_LENGTH


def mdct_num_frames(T: int, frame_period: int) -> int:
    """Frames of mdct.py:175-176: the signal padded by P on the right, centred frames of hop P."""
    return (T + frame_period - 1) // frame_period + 1


def mdct_out_length(N: int, frame_period: int, out_length) -> int:
    """imdct.py:178-181 over unframe.py:164-211."""
    return max(0, (N - 1) * frame_period) if out_length is None else max(0, min(int(out_length), N * frame_period))


def _transform_code(transform: str) -> int:
    try:
        return MDCT_TRANSFORMS[transform]
    except KeyError:
        raise ValueError(f"transform must be either 'cosine' or 'sine'. Got '{transform}'.") from None


def _analysis(x, N, w, table, z, transform, scale):
    """x:(..., T) -> (..., N, P); table: the twiddles where the fast kernels run, else the (L, P) basis."""
    L = w.numel()
    P = L // 2
    xc = x.contiguous()
    T = xc.size(-1)
    B = xc.numel() // max(T, 1)
    fast = mdct_fast_supported(L, xc.dtype)
    y = torch.empty(*xc.shape[:-1], N, P, device=xc.device, dtype=xc.dtype)
    with torch.cuda.device(xc.device):
        _call("dsa_mdct_analysis", _p(xc), B, T, N, L, _p(w), None if fast else _p(table), _p(table) if fast else None, float(z), transform,
              scale, _dtype_code(xc), _lib.ALGO_AUTO, _p(y), _stream())
    return y


def _synthesis(y, T, w, table, z, transform, scale):
    """y:(..., N, P) -> (..., T); table: the twiddles where the fast kernels run, else the (P, L) transposed basis."""
    L = w.numel()
    yc = y.contiguous()
    N = yc.size(-2)
    B = yc.numel() // max(N * (L // 2), 1)
    fast = mdct_fast_supported(L, yc.dtype)
    x = torch.empty(*yc.shape[:-2], T, device=yc.device, dtype=yc.dtype)
    with torch.cuda.device(yc.device):
        _call("dsa_mdct_synthesis", _p(yc), B, N, L, _p(w), None if fast else _p(table), _p(table) if fast else None, float(z), transform,
              scale, T, _dtype_code(yc), _lib.ALGO_AUTO, _p(x), _stream())
    return x


def _check_tables(op, t, w, table_a, table_s):
    _require_device(t, w, table_a, table_s)
    _same_dtype(t, w, table_a, table_s)
    L = w.numel()
    if L < 2 or L % 2:
        raise ValueError("length must be at least 2 and even.")
    fast = mdct_fast_supported(L, t.dtype)
    want_a, want_s = ((3 * L // 4,), (3 * L // 4,)) if fast else ((L, L // 2), (L // 2, L))
    if tuple(table_a.shape) != want_a or tuple(table_s.shape) != want_s or not (table_a.is_contiguous() and table_s.is_contiguous() and w.is_contiguous()):
        raise ValueError(f"{op}: tables {tuple(table_a.shape)}, {tuple(table_s.shape)} do not fit frame length {L} in {t.dtype}")


class MdctFn(torch.autograd.Function):
    """x:(..., T) -> y:(..., N, L/2), N = (T + P - 1) // P + 1 (mdct.py:166-176).  w:(L); table_a / table_s: what the analysis and the
    synthesis kernels read (utils.tables.mdct_twiddle twice where mdct_fast_supported, else mdct_basis and its transpose).  The backward
    is the synthesis without the overlap division; nothing is saved."""

    @staticmethod
    def forward(ctx, x, w, table_a, table_s, z, transform):
        _check_tables("mdct", x, w, table_a, table_s)
        code = _transform_code(transform)
        if x.dim() < 1 or x.size(-1) < 1:
            raise ValueError("mdct: the input needs at least one sample.")
        ctx.cfg = (w, table_s, z, code, x.size(-1))
        return _analysis(x, mdct_num_frames(x.size(-1), w.numel() // 2), w, table_a, z, code, _lib.MDCT_SCALE_NONE)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        w, table_s, z, code, T = ctx.cfg
        return _synthesis(gy, T, w, table_s, z, code, _lib.MDCT_SCALE_NONE), None, None, None, None, None


class ImdctFn(torch.autograd.Function):
    """y:(..., N, L/2) -> x:(..., T_out), T_out = (N - 1) P, or min(out_length, N P) (imdct.py:169-181): overlap-add divided by the number
    of frames over each sample.  The backward is the analysis of the cotangent with that division applied on load; nothing is saved."""

    @staticmethod
    def forward(ctx, y, out_length, w, table_a, table_s, z, transform):
        _check_tables("imdct", y, w, table_a, table_s)
        code = _transform_code(transform)
        if y.dim() <= 1:
            raise ValueError("Input must be at least 2D tensor.")   # unframe.py
        P = w.numel() // 2
        if y.size(-1) != P:
            raise ValueError(f"Unexpected dimension of input (input {y.size(-1)} vs target {P}).")
        N = y.size(-2)
        ctx.cfg = (w, table_a, z, code, N)
        return _synthesis(y, mdct_out_length(N, P, out_length), w, table_s, z, code, _lib.MDCT_SCALE_OVERLAP)

    @staticmethod
    @once_differentiable
    def backward(ctx, gx):
        w, table_a, z, code, N = ctx.cfg
        if gx.size(-1) == 0 or N == 0:
            return gx.new_zeros(*gx.shape[:-1], N, w.numel() // 2), None, None, None, None, None, None
        return _analysis(gx, N, w, table_a, z, code, _lib.MDCT_SCALE_OVERLAP), None, None, None, None, None, None
