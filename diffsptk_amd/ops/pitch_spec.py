"""The pitch-adaptive spectral envelope of CheapTrick (csrc/pitch_spec.hip): a frame from the waveform to the formatted envelope in one
launch, and the adjoint down to the waveform in two."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ._core import _call, _dtype_code, _p, _require_device, _same_dtype, _stream, num_frames

PITCH_SPEC_FORMATS = {0: 0, "db": 0, 1: 1, "log-magnitude": 1, 2: 2, "magnitude": 2, 3: 3, "power": 3}


def pitch_spec_lds_bytes(fft_length: int) -> int:
    """DSA_PITCH_SPEC_LDS_BYTES(L) of include/diffsptk_amd.h, section a26: in float64 the transform's two arrays of L, the kept spectrum
    (2 (L / 2 + 1)), the smoothed spectrum (L / 2 + 1) and 32 words for the reductions"""
    return 28 * fft_length + 280


def check_pitch_spec_length(fft_length: int) -> None:
    """The two ceilings of the per-frame workgroup, by the name of the constant; needs no device."""
    if fft_length < 16 or fft_length & (fft_length - 1):
        raise ValueError(f"pitch_spec: fft_length {fft_length} is not a power of two: the per-frame workgroup of diffsptk_amd transforms in LDS by "
                         "radix 2 (the reference takes any length of at least 1024; WORLD itself uses powers of two)")
    need = pitch_spec_lds_bytes(fft_length)
    if need > _lib.PITCH_SPEC_MAX_LDS_BYTES:
        raise ValueError(f"pitch_spec: fft_length {fft_length} takes DSA_PITCH_SPEC_LDS_BYTES = {need} bytes per frame: the transform, the kept "
                         f"spectrum and the smoothed spectrum must fit DSA_PITCH_SPEC_MAX_LDS_BYTES = {_lib.PITCH_SPEC_MAX_LDS_BYTES} bytes of LDS "
                         "(fft_length <= 4096)")


class PitchSpecFn(torch.autograd.Function):
    """x:(B, T), f0:(B, N), noise1:(B, N, L) or None, noise2:(B, N, L / 2 + 1) or None, twiddle:(L, 2) float64 -> y:(B, N, L / 2 + 1).
    cfg = (P, sample_rate, L, default_f0, q1, eps, floor_ratio, format).  Saved for the backward: the inputs and the two noise tensors; the
    forward is run again."""

    @staticmethod
    def forward(ctx, x, f0, noise1, noise2, twiddle, cfg):
        P, sr, L, default_f0, q1, eps, floor_ratio, fmt = cfg
        check_pitch_spec_length(L)
        B, T = x.shape
        N = f0.shape[1]
        if f0.shape[0] != B:
            raise ValueError("x and f0 must have the same batch size.")
        if N != num_frames(T, P):
            raise ValueError(f"f0 must have (T - 1) // frame_period + 1 = {num_frames(T, P)} frames for a waveform of {T} samples, got {N}.")
        _same_dtype(x, f0, noise1, noise2)
        code = _dtype_code(x)
        _require_device(x, f0, noise1, noise2, twiddle)
        if twiddle.dtype != torch.float64 or tuple(twiddle.shape) != (L, 2):
            raise ValueError("pitch_spec: the twiddle table is (fft_length, 2) float64 whatever the data's dtype")
        K = L // 2 + 1
        xc, fc = x.contiguous(), f0.detach().contiguous()
        n1 = None if noise1 is None else noise1.contiguous()
        n2 = None if noise2 is None else noise2.contiguous()
        if (n1 is not None and tuple(n1.shape) != (B, N, L)) or (n2 is not None and tuple(n2.shape) != (B, N, K)):
            raise ValueError("pitch_spec: the noise tensors are (B, N, fft_length) and (B, N, fft_length / 2 + 1)")
        y = torch.empty(B, N, K, device=x.device, dtype=x.dtype)
        if B and N:
            with torch.cuda.device(x.device):
                _call("dsa_pitch_spec", _p(xc), _p(fc), _p(n1), _p(n2), _p(twiddle), B, N, T, P, sr, L, float(default_f0), float(q1), float(eps),
                      float(floor_ratio), fmt, code, _p(y), _stream())
        ctx.cfg = cfg
        ctx.save_for_backward(xc, fc, n1, n2, twiddle)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xc, fc, n1, n2, twiddle = ctx.saved_tensors
        P, sr, L, default_f0, q1, eps, floor_ratio, fmt = ctx.cfg
        (B, T), N = xc.shape, fc.shape[1]
        code = _dtype_code(xc)
        gx = torch.empty_like(xc)
        if B and N:
            gc = gy.contiguous()
            with torch.cuda.device(xc.device):
                gframes = torch.empty(B, N, L, device=xc.device, dtype=torch.float64)
                _call("dsa_pitch_spec_vjp_frames", _p(gc), _p(xc), _p(fc), _p(n1), _p(n2), _p(twiddle), B, N, T, P, sr, L, float(default_f0),
                      float(q1), float(eps), float(floor_ratio), fmt, code, _p(gframes), _stream())
                _call("dsa_pitch_spec_vjp_gather", _p(gframes), B, N, T, P, L, code, _p(gx), _stream())
        return gx, None, None, None, None, None
