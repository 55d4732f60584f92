"""FFT cepstrum, mel filter bank (alone, behind the STFT, under MFCC), PLP: csrc/fftcep.hip, fbank.hip, plp.hip (+ stft.hip)."""
from __future__ import annotations

import weakref

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ._core import _call, _dtype_code, _p, _require_device, _same_dtype, _stream, num_frames, pad_mode_code


class FftcepFn(torch.autograd.Function):
    """CepstralAnalysis._forward (fftcep.py:116-136): x:(..., L/2+1) power spectra -> (..., M+1)."""

    @staticmethod
    def forward(ctx, x, A, cep_order, accel, n_iter):
        _require_device(x, A)
        _same_dtype(x, A)
        xc, Ac = x.contiguous(), A.contiguous()
        H = xc.size(-1)
        L = 2 * (H - 1)
        F = xc.numel() // H
        out = torch.empty(*xc.shape[:-1], cep_order + 1, device=x.device, dtype=x.dtype)
        masks = None
        if n_iter > 0 and x.requires_grad:
            masks = torch.empty(F, n_iter, (H + 63) // 64, device=x.device, dtype=torch.int64)
        with torch.cuda.device(x.device):
            _call("dsa_fftcep_fwd", _p(xc), F, L, cep_order, _p(Ac), float(accel), n_iter, _dtype_code(xc), _p(out),
                  _p(masks) if masks is not None else None, _stream())
        ctx.save_for_backward(xc, Ac, masks)
        ctx.cfg = (L, cep_order, float(accel), n_iter)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        xc, Ac, masks = ctx.saved_tensors
        L, M, accel, n_iter = ctx.cfg
        H = xc.size(-1)
        F = xc.numel() // H
        gc = g.contiguous()
        gx = torch.empty_like(xc)
        with torch.cuda.device(g.device):
            _call("dsa_fftcep_bwd", _p(gc), _p(xc), F, L, M, _p(Ac), accel, n_iter, _p(masks) if masks is not None else None,
                  _dtype_code(xc), _p(gx), _stream())
        return gx, None, None, None, None


class FbankFn(torch.autograd.Function):
    """y, E = mel filter bank outputs and log energy of power spectra (fbank.py:306-321).
    H is a fixed matrix here (a learnable basis is not supported by the kernels)."""

    @staticmethod
    def forward(ctx, x, H, floor, gamma, use_power):
        _require_device(x, H)
        _same_dtype(x, H)
        xc, Hc = x.contiguous(), H.contiguous()
        K, Cn = Hc.shape
        F = xc.numel() // K
        y = torch.empty(*xc.shape[:-1], Cn, device=x.device, dtype=x.dtype)
        E = torch.empty(*xc.shape[:-1], 1, device=x.device, dtype=x.dtype)
        with torch.cuda.device(x.device):
            _call("dsa_fbank_fwd", _p(xc), F, K, _p(Hc), Cn, float(floor), float(gamma), int(bool(use_power)),
                  _dtype_code(xc), _p(y), _p(E), _stream())
        ctx.save_for_backward(xc, Hc)
        ctx.cfg = (float(floor), float(gamma), int(bool(use_power)))
        return y, E

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, gE):
        xc, Hc = ctx.saved_tensors
        floor, gamma, use_power = ctx.cfg
        K, Cn = Hc.shape
        F = xc.numel() // K
        gyc = gy.contiguous() if gy is not None else torch.zeros(*xc.shape[:-1], Cn, device=xc.device, dtype=xc.dtype)
        gEc = gE.contiguous() if gE is not None else None
        gx = torch.empty_like(xc)
        with torch.cuda.device(xc.device):
            _call("dsa_fbank_bwd", _p(gyc), _p(gEc) if gEc is not None else None, _p(xc), F, K, _p(Hc), Cn, floor, gamma,
                  use_power, _dtype_code(xc), _p(gx), _stream())
        return gx, None, None, None, None


_FB_PLANS: dict = {}   # id(H) -> (weakref to H, version, plan or None)


def fbank_scan_plan(H: torch.Tensor):
    """The per-lane plan of the fused STFT -> filter-bank kernel for the (257, C) weights `H` (dsa_fbank_scan_plan: built
    on the host, one device-to-host copy of H per matrix and version), as a device tensor -- or None when H does not
    have the two-adjacent-channels-per-bin structure the kernel sums over (the two-kernel path serves those)."""
    import numpy as np

    key = id(H)
    hit = _FB_PLANS.get(key)
    if hit is not None and hit[0]() is H and hit[1] == H._version:
        return hit[2]
    plan = None
    if H.dim() == 2 and H.size(0) == 257 and 1 <= H.size(1) <= 126:
        Hh = np.ascontiguousarray(H.detach().to("cpu", torch.float64).numpy())
        table = np.zeros(_lib.FBANK_PLAN_FLOATS, dtype=np.float32)
        rc = _lib.load().dsa_fbank_scan_plan(Hh.ctypes.data, 257, int(H.size(1)), table.ctypes.data)
        if rc == 0:
            plan = torch.from_numpy(table).to(H.device)
        elif rc != _lib.ERR_UNSUPPORTED:
            _lib.check(rc, "dsa_fbank_scan_plan")
    _FB_PLANS[key] = (weakref.ref(H), H._version, plan)
    weakref.finalize(H, _FB_PLANS.pop, key, None)
    return plan


def stft_fbank(x, window, twiddle, L, P, fft_length, center, eps, plan, n_channel, floor, gamma, use_power):
    """y:(..., N, C) = glog(max(s H, floor)) of the STFT power values (or their square roots) in ONE launch
    (dsa_stft_fbank_fwd: stft.py:148-152 + fbank.py:306-321); no autograd graph (StftFbankFn wraps it with one)."""
    _require_device(x, window, twiddle, plan)
    _same_dtype(x, window, twiddle)
    xc, wc = x.contiguous(), window.contiguous()
    T = xc.size(-1)
    B = xc.numel() // T if T > 0 else 0
    y = torch.empty((*xc.shape[:-1], num_frames(T, P), n_channel), device=x.device, dtype=x.dtype)
    with torch.cuda.device(x.device):
        _call("dsa_stft_fbank_fwd", _p(xc), B, T, L, P, fft_length, _p(wc), _p(twiddle), int(center), float(eps), _p(plan),
              int(n_channel), float(floor), float(gamma), int(bool(use_power)), _dtype_code(xc), _p(y), _stream())
    return y


_BINS_TABLES: dict = {}   # id(H) -> (weakref to H, version, table or None)


def fbank_bins_table(H: torch.Tensor):
    """Device table of dsa_fbank_bins_bwd for the filter-bank matrix H (dsa_fbank_bins_plan: built on the host, once per
    matrix and version) -- or None when a bin feeds more than two adjacent channels."""
    import numpy as np

    key = id(H)
    hit = _BINS_TABLES.get(key)
    if hit is not None and hit[0]() is H and hit[1] == H._version:
        return hit[2]
    t = None
    if H.dim() == 2:
        Hh = np.ascontiguousarray(H.detach().to("cpu", torch.float64).numpy())
        table = np.zeros(4 * H.size(0), dtype=np.float32)
        if _lib.load().dsa_fbank_bins_plan(Hh.ctypes.data, int(H.size(0)), int(H.size(1)), table.ctypes.data) == 0:
            t = torch.from_numpy(table).to(H.device)
    if hit is None or hit[0]() is not H:
        weakref.finalize(H, _BINS_TABLES.pop, key, None)   # the table goes when the matrix goes
    _BINS_TABLES[key] = (weakref.ref(H), H._version, t)
    return t


class StftFbankFn(torch.autograd.Function):
    """stft_fbank with a gradient.  Forward: the one-launch kernel (the spectrogram never exists).  Backward, two launches:
    dsa_fbank_bins_bwd spreads the channel cotangents times d glog / d s (from the SAVED OUTPUT; 0 where the floor clamped, as
    torch.clip does in fbank.py:312) over the bins -- two multiply-adds per bin, the matrix has two entries per row -- and the
    result enters dsa_stft_bwd as the cotangent of the power / magnitude spectrum (which it recomputes from the waveform)."""

    @staticmethod
    def forward(ctx, x, window, twiddle, H, plan, L, P, fft_length, center, eps, floor, gamma, use_power):
        y = stft_fbank(x, window, twiddle, L, P, fft_length, center, eps, plan, H.size(1), floor, gamma, use_power)
        ctx.save_for_backward(x.contiguous(), window.contiguous(), twiddle, fbank_bins_table(H), y)
        ctx.cfg = (L, P, fft_length, center, eps, floor, gamma, use_power, H.size(0), H.size(1))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xc, wc, twiddle, table, y = ctx.saved_tensors
        L, P, fft_length, center, eps, floor, gamma, use_power, K, Cn = ctx.cfg
        gy = gy.contiguous()
        F = gy.numel() // Cn
        g = torch.empty(*gy.shape[:-1], K, device=gy.device, dtype=gy.dtype)
        T = xc.size(-1)
        B = xc.numel() // T
        gx = torch.empty_like(xc)
        with torch.cuda.device(gy.device):
            _call("dsa_fbank_bins_bwd", _p(gy), _p(y), F, K, Cn, _p(table), float(floor), float(gamma), _dtype_code(gy), _p(g),
                  _stream())
            _call("dsa_stft_bwd", _p(g), _p(xc), B, T, L, P, fft_length, _p(wc), _p(twiddle), int(center), 0,
                  pad_mode_code("constant"), float(eps), 0, 0.0, 3 if use_power else 2, _dtype_code(xc), _lib.ALGO_AUTO,
                  _p(gx), None, _stream())
        return (gx,) + (None,) * 12


class MfccFn(torch.autograd.Function):
    """cy, E = (glog(max(s H, floor)) W, log energy) in one launch (mfcc.py:244-256): W:(C, M+1) is DCT-II x truncation
    x liftering vector.  Backward = the transposed product through W, then the filter-bank backward."""

    @staticmethod
    def forward(ctx, x, H, W, floor, gamma, use_power):
        _require_device(x, H, W)
        _same_dtype(x, H)
        _same_dtype(x, W)
        xc, Hc, Wc = x.contiguous(), H.contiguous(), W.contiguous()
        K, Cn = Hc.shape
        Mo = Wc.size(1)
        F = xc.numel() // K
        z = torch.empty(*xc.shape[:-1], Mo, device=x.device, dtype=x.dtype)
        E = torch.empty(*xc.shape[:-1], 1, device=x.device, dtype=x.dtype)
        with torch.cuda.device(x.device):
            _call("dsa_fbank_dct_fwd", _p(xc), F, K, _p(Hc), Cn, _p(Wc), Mo, float(floor), float(gamma), int(bool(use_power)),
                  _dtype_code(xc), _p(z), _p(E), _stream())
        ctx.save_for_backward(xc, Hc, Wc)
        ctx.cfg = (float(floor), float(gamma), int(bool(use_power)))
        return z, E

    @staticmethod
    @once_differentiable
    def backward(ctx, gz, gE):
        xc, Hc, Wc = ctx.saved_tensors
        floor, gamma, use_power = ctx.cfg
        K, Cn = Hc.shape
        Mo = Wc.size(1)
        F = xc.numel() // K
        gy = torch.empty(*xc.shape[:-1], Cn, device=xc.device, dtype=xc.dtype)
        gx = torch.empty_like(xc)
        gEc = gE.contiguous() if gE is not None else None
        with torch.cuda.device(xc.device):
            if gz is not None:
                _call("dsa_freqt_bwd", _p(gz.contiguous()), F, Cn, _p(Wc), Mo, _dtype_code(xc), _p(gy), _stream())
            else:
                gy.zero_()
            _call("dsa_fbank_bwd", _p(gy), _p(gEc) if gEc is not None else None, _p(xc), F, K, _p(Hc), Cn, floor, gamma,
                  use_power, _dtype_code(xc), _p(gx), _stream())
        return gx, None, None, None, None, None


PLP_FORMATS = {"y": 0, "yE": 1, "yc": 2, "ycE": 3}


class PlpFn(torch.autograd.Function):
    """PLP after the filter bank (plp.py:315-320): y:(..., C) log filter-bank outputs and E:(..., 1) (None unless out_format
    carries it) -> (..., M + {0, 1, 1, 2}).  Equal loudness, compression, replicate1, hfft, Levinson (eps = 0), the n_fft-point
    LPC -> cepstrum sum, lifter and formatter in one launch (dsa_plp_fwd); the adjoint of all of it in one launch (dsa_plp_bwd)
    from the saved [K, a].  `table` is the packed constant table (tables.plp_table) in the dtype of y."""

    @staticmethod
    def forward(ctx, y, E, table, M, n_fft, compression_factor, fmt):
        _require_device(y, E, table)
        _same_dtype(y, E, table)
        code = PLP_FORMATS[fmt]
        if (code & 1) and E is None:
            raise ValueError(f"plp: out_format {fmt} needs E")
        yc = y.contiguous()
        Ec = E.contiguous() if code & 1 else None
        C = yc.size(-1)
        F = yc.numel() // C
        Mo = M + (code & 1) + (code >> 1)
        out = torch.empty(*yc.shape[:-1], Mo, device=y.device, dtype=y.dtype)
        save = torch.empty(F, M + 1, device=y.device, dtype=y.dtype) if ctx.needs_input_grad[0] else None
        with torch.cuda.device(y.device):
            _call("dsa_plp_fwd", _p(yc), _p(Ec), F, C, M, n_fft, float(compression_factor), code, _p(table), _dtype_code(yc),
                  _p(out), _p(save), _stream())
        ctx.save_for_backward(yc, table, save)
        ctx.cfg = (M, n_fft, float(compression_factor), code, E is not None)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        yc, table, save = ctx.saved_tensors
        M, n_fft, cf, code, has_E = ctx.cfg
        C = yc.size(-1)
        F = yc.numel() // C
        gy = torch.empty_like(yc)
        gE = torch.empty(*yc.shape[:-1], 1, device=yc.device, dtype=yc.dtype) if has_E and ctx.needs_input_grad[1] else None
        with torch.cuda.device(yc.device):
            _call("dsa_plp_bwd", _p(gout.contiguous()), _p(yc), _p(save), F, C, M, n_fft, cf, code, _p(table), _dtype_code(yc),
                  _p(gy), _p(gE), _stream())
        return gy, gE, None, None, None, None, None
