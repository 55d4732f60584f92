"""Yingram (csrc/yingram.hip): YIN's cumulative-mean-normalised difference function on a semitone grid, forward and adjoint, from frames
or from the waveform in one launch."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ._core import _call, _dtype_code, _p, _require_device, _same_dtype, _stream, num_frames, pad_mode_code


def yingram_fft_length(L: int, lag_max: int) -> int:
    """2 H of include/diffsptk_amd.h, section a22: the power of two from L + lag_max on (at least 4) whose twiddle table the fft route reads"""
    n = 4
    while n < L + lag_max:
        n *= 2
    return n


def yingram_lds_bytes(L: int, size: int) -> int:
    """DSA_YINGRAM_LDS_BYTES(H, L, size) at the H of the longest lag range, lag_max = L - 1: the transform's two arrays of H values, one
    more of H + 1, L + 1 float64 prefix sums and the scan's exchange -- what the fft route's workgroup holds in LDS"""
    H = yingram_fft_length(L, L - 1) // 2
    return (3 * H + 1) * size + 8 * (L + 1) + 128


def _check_yingram(x, L, lag_max, lags, lags_floor, lags_ceil, twiddle, what="x"):
    """The ceiling first, the device last."""
    if x.dim() < 1 or not 1 <= lag_max < L:
        raise ValueError(f"yingram: {what} must be (..., L) with 1 <= lag_max < L, got {tuple(x.shape)} and lag_max = {lag_max}")
    if not (lags.dim() == 1 and lags_floor.shape == lags.shape == lags_ceil.shape and lags_floor.dtype == lags_ceil.dtype == torch.int64):
        raise ValueError("yingram: lags, lags_floor and lags_ceil must be (M,) tables, the last two int64")
    need = yingram_lds_bytes(L, x.element_size())
    if need > _lib.YINGRAM_MAX_LDS_BYTES:
        raise ValueError(f"yingram: frames of {L} samples take {need} bytes: the transform of twice the frame, the difference function and the "
                         f"energy prefix sums must fit DSA_YINGRAM_MAX_LDS_BYTES = {_lib.YINGRAM_MAX_LDS_BYTES} bytes of LDS")
    _same_dtype(x, lags, twiddle)
    _dtype_code(x)
    _require_device(x, lags, lags_floor, lags_ceil, twiddle)


def _yingram_bwd(gy, xc, L, lag_max, lags, fl, ce, twiddle, algo):
    """gx:(F, L) of frames xc:(F, L) (contiguous) for the cotangent gy:(F, M)"""
    gc = gy.contiguous()
    gx = torch.empty_like(xc)
    F = xc.numel() // L
    if F:
        with torch.cuda.device(xc.device):
            _call("dsa_yingram_vjp", _p(gc), _p(xc), F, L, lag_max, _p(lags), _p(fl), _p(ce), lags.numel(), _p(twiddle), algo, _dtype_code(xc),
                  _p(gx), _stream())
    return gx


class YingramFn(torch.autograd.Function):
    """x:(..., L) -> (..., M) for the tables of Yingram._precompute (lags of x's dtype, the other two int64) and the twiddle table of
    yingram_fft_length(L, lag_max) points (modules/spec.py: device_twiddle).  algo: _lib.ALGO_AUTO / ALGO_GENERIC (direct) / ALGO_TUNED
    (fft).  Saved for the backward: x and the tables.  No host read."""

    @staticmethod
    def forward(ctx, x, lags, lags_floor, lags_ceil, twiddle, lag_max, algo):
        L = x.size(-1) if x.dim() else 0
        _check_yingram(x, L, lag_max, lags, lags_floor, lags_ceil, twiddle)
        xc, lc, fc, cc = x.contiguous(), lags.contiguous(), lags_floor.contiguous(), lags_ceil.contiguous()
        M = lc.numel()
        F = xc.numel() // L
        y = torch.empty(*xc.shape[:-1], M, device=xc.device, dtype=xc.dtype)
        if F and M:
            with torch.cuda.device(xc.device):
                _call("dsa_yingram", _p(xc), F, L, lag_max, _p(lc), _p(fc), _p(cc), M, _p(twiddle), algo, _dtype_code(xc), _p(y), _stream())
        ctx.cfg = (L, lag_max, algo)
        ctx.save_for_backward(xc, lc, fc, cc, twiddle)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xc, lc, fc, cc, twiddle = ctx.saved_tensors
        L, lag_max, algo = ctx.cfg
        return _yingram_bwd(gy, xc, L, lag_max, lc, fc, cc, twiddle, algo), None, None, None, None, None, None


class FrameYingramFn(torch.autograd.Function):
    """x:(..., T) -> (..., N, M): YingramFn on Frame(L, P, center) of x (constant padding, no zmean) in one launch, the frames never in
    memory.  The backward frames x again (dsa_frame_fwd), runs dsa_yingram_vjp on the frames and folds their cotangent (dsa_frame_bwd)."""

    @staticmethod
    def forward(ctx, x, lags, lags_floor, lags_ceil, twiddle, L, P, center, lag_max, algo):
        _check_yingram(x, L, lag_max, lags, lags_floor, lags_ceil, twiddle, what="the frames of x")
        xc, lc, fc, cc = x.contiguous(), lags.contiguous(), lags_floor.contiguous(), lags_ceil.contiguous()
        T = xc.size(-1)
        B = xc.numel() // T if T > 0 else 0
        N, M = num_frames(T, P), lc.numel()
        y = torch.empty(*xc.shape[:-1], N, M, device=xc.device, dtype=xc.dtype)
        if B and N and M:
            with torch.cuda.device(xc.device):
                _call("dsa_frame_yingram", _p(xc), B, T, L, P, int(center), lag_max, _p(lc), _p(fc), _p(cc), M, _p(twiddle), algo,
                      _dtype_code(xc), _p(y), _stream())
        ctx.cfg = (L, P, bool(center), lag_max, algo)
        ctx.save_for_backward(xc, lc, fc, cc, twiddle)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xc, lc, fc, cc, twiddle = ctx.saved_tensors
        L, P, center, lag_max, algo = ctx.cfg
        T = xc.size(-1)
        B = xc.numel() // T if T > 0 else 0
        N = num_frames(T, P)
        gx = torch.empty_like(xc)
        if B and N:
            code, pad = _dtype_code(xc), pad_mode_code("constant")
            frames = torch.empty(B * N, L, device=xc.device, dtype=xc.dtype)
            with torch.cuda.device(xc.device):
                _call("dsa_frame_fwd", _p(xc), B, T, L, P, int(center), 0, pad, code, _p(frames), _stream())
                gf = _yingram_bwd(gy, frames, L, lag_max, lc, fc, cc, twiddle, algo)
                _call("dsa_frame_bwd", _p(gf), B, T, L, P, int(center), 0, pad, code, _p(gx), _stream())
        return gx, None, None, None, None, None, None, None, None, None
