"""Frame, Window, fftr, Spectrum, STFT and the inverse path (ifftr, Unframe, ISTFT, Griffin-Lim): csrc/spec.hip, stft.hip, griffin.hip."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from ._core import _call, _dtype_code, _p, _require_device, _same_dtype, _stream, num_frames, pad_mode_code

# ----------------------------------------------------------------------------------- Frame
class FrameFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, L, P, center, zmean, mode):
        _require_device(x)
        xc = x.contiguous()
        T = xc.size(-1)
        B = xc.numel() // T if T > 0 else 0
        N = num_frames(T, P)
        y = torch.empty(*xc.shape[:-1], N, L, device=x.device, dtype=x.dtype)
        with torch.cuda.device(x.device):
            _call("dsa_frame_fwd", _p(xc), B, T, L, P, int(center), int(zmean), pad_mode_code(mode),
                  _dtype_code(xc), _p(y), _stream())
        ctx.cfg = (xc.shape, L, P, center, zmean, mode)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        shape, L, P, center, zmean, mode = ctx.cfg
        gy = gy.contiguous()
        T = shape[-1]
        B = gy.numel() // (num_frames(T, P) * L)
        gx = torch.empty(shape, device=gy.device, dtype=gy.dtype)
        with torch.cuda.device(gy.device):
            _call("dsa_frame_bwd", _p(gy), B, T, L, P, int(center), int(zmean), pad_mode_code(mode),
                  _dtype_code(gy), _p(gx), _stream())
        return gx, None, None, None, None, None


# ----------------------------------------------------------------------------------- Window
class WindowFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, out_length):
        _require_device(x, w)
        _same_dtype(x, w)
        xc, wc = x.contiguous(), w.contiguous()
        L = xc.size(-1)
        L2 = L if out_length is None else out_length
        F = xc.numel() // L
        y = torch.empty(*xc.shape[:-1], L2, device=x.device, dtype=x.dtype)
        with torch.cuda.device(x.device):
            _call("dsa_window_fwd", _p(xc), F, L, _p(wc), L2, _dtype_code(xc), _p(y), _stream())
        ctx.save_for_backward(xc, wc)
        ctx.L2 = L2
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xc, wc = ctx.saved_tensors
        gy = gy.contiguous()
        L = xc.size(-1)
        F = xc.numel() // L
        gx = torch.empty_like(xc)
        gw = torch.empty_like(wc) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(gy.device):
            _call("dsa_window_bwd", _p(gy), _p(xc), F, L, _p(wc), ctx.L2, _dtype_code(xc), _p(gx), _p(gw),
                  _stream())
        return gx, gw, None


# ----------------------------------------------------------------------------------- fftr
class FftrFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fft_length, fmt, twiddle):
        _require_device(x, twiddle)
        _same_dtype(x, twiddle)
        xc = x.contiguous()
        len_in = xc.size(-1)
        F = xc.numel() // len_in
        K = fft_length // 2 + 1
        shape = (*xc.shape[:-1], K, 2) if fmt == 0 else (*xc.shape[:-1], K)
        y = torch.empty(shape, device=x.device, dtype=x.dtype)
        with torch.cuda.device(x.device):
            _call("dsa_fftr_fwd", _p(xc), F, len_in, fft_length, fmt, _p(twiddle), _dtype_code(xc), _p(y),
                  _stream())
        ctx.save_for_backward(xc, twiddle)
        ctx.cfg = (fft_length, fmt)
        return torch.view_as_complex(y) if fmt == 0 else y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xc, twiddle = ctx.saved_tensors
        fft_length, fmt = ctx.cfg
        if fmt == 0:
            gy = torch.view_as_real(gy.resolve_conj())
        gy = gy.contiguous()
        len_in = xc.size(-1)
        F = xc.numel() // len_in
        gx = torch.empty_like(xc)
        with torch.cuda.device(gy.device):
            _call("dsa_fftr_bwd", _p(gy), _p(xc), F, len_in, fft_length, fmt, _p(twiddle), _dtype_code(xc),
                  _p(gx), _stream())
        return gx, None, None, None


# ----------------------------------------------------------------------------------- Spectrum
class SpecFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, b, a, fft_length, eps, relative_floor_db, fmt, twiddle):
        ref = b if b is not None else a
        _require_device(b, a, twiddle)
        _same_dtype(ref, b, a, twiddle)
        bc = b.contiguous() if b is not None else None
        ac = a.contiguous() if a is not None else None
        lb = bc.size(-1) if bc is not None else 0
        la = ac.size(-1) if ac is not None else 0
        F = ref.numel() // ref.size(-1)
        K = fft_length // 2 + 1
        y = torch.empty(*ref.shape[:-1], K, device=ref.device, dtype=ref.dtype)
        use_floor = relative_floor_db is not None
        with torch.cuda.device(ref.device):
            _call("dsa_spec_fwd", _p(bc), lb, _p(ac), la, F, fft_length, float(eps), int(use_floor),
                  float(relative_floor_db or 0.0), fmt, _p(twiddle), _dtype_code(ref), _p(y), _stream())
        ctx.save_for_backward(bc, ac, twiddle)
        ctx.cfg = (fft_length, eps, relative_floor_db, fmt)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        bc, ac, twiddle = ctx.saved_tensors
        fft_length, eps, relative_floor_db, fmt = ctx.cfg
        gy = gy.contiguous()
        ref = bc if bc is not None else ac
        F = ref.numel() // ref.size(-1)
        gb = torch.empty_like(bc) if bc is not None else None
        ga = torch.empty_like(ac) if ac is not None else None
        use_floor = relative_floor_db is not None
        with torch.cuda.device(gy.device):
            _call("dsa_spec_bwd", _p(gy), _p(bc), bc.size(-1) if bc is not None else 0, _p(ac),
                  ac.size(-1) if ac is not None else 0, F, fft_length, float(eps), int(use_floor),
                  float(relative_floor_db or 0.0), fmt, _p(twiddle), _dtype_code(ref), _p(gb), _p(ga), _stream())
        return gb, ga, None, None, None, None, None


# ----------------------------------------------------------------------------------- STFT
class StftFn(torch.autograd.Function):
    """Fused Frame + Window + rFFT + Spectrum formatter (stft.py:237-241)."""

    @staticmethod
    def forward(ctx, x, window, twiddle, L, P, fft_length, center, zmean, mode, eps, relative_floor_db, fmt,
                algo):
        _require_device(x, window, twiddle)
        _same_dtype(x, window, twiddle)
        xc, wc = x.contiguous(), window.contiguous()
        T = xc.size(-1)
        B = xc.numel() // T if T > 0 else 0
        N = num_frames(T, P)
        K = fft_length // 2 + 1
        shape = (*xc.shape[:-1], N, K, 2) if fmt == 4 else (*xc.shape[:-1], N, K)
        y = torch.empty(shape, device=x.device, dtype=x.dtype)
        use_floor = relative_floor_db is not None
        with torch.cuda.device(x.device):
            _call("dsa_stft_fwd", _p(xc), B, T, L, P, fft_length, _p(wc), _p(twiddle), int(center), int(zmean),
                  pad_mode_code(mode), float(eps), int(use_floor), float(relative_floor_db or 0.0), fmt,
                  _dtype_code(xc), algo, _p(y), _stream())
        ctx.save_for_backward(xc, wc, twiddle)
        ctx.cfg = (L, P, fft_length, center, zmean, mode, eps, relative_floor_db, fmt, algo)
        return torch.view_as_complex(y) if fmt == 4 else y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xc, wc, twiddle = ctx.saved_tensors
        L, P, fft_length, center, zmean, mode, eps, relative_floor_db, fmt, algo = ctx.cfg
        if fmt == 4:
            gy = torch.view_as_real(gy.resolve_conj())
        gy = gy.contiguous()
        T = xc.size(-1)
        B = xc.numel() // T
        gx = torch.empty_like(xc)
        gw = torch.empty_like(wc) if ctx.needs_input_grad[1] else None
        use_floor = relative_floor_db is not None
        with torch.cuda.device(gy.device):
            _call("dsa_stft_bwd", _p(gy), _p(xc), B, T, L, P, fft_length, _p(wc), _p(twiddle), int(center),
                  int(zmean), pad_mode_code(mode), float(eps), int(use_floor), float(relative_floor_db or 0.0),
                  fmt, _dtype_code(xc), algo, _p(gx), _p(gw), _stream())
        return (gx, gw) + (None,) * 11


# ----------------------------------------------------------------------------------- inverse path (8(f) row 2)
# irfft = adjoint of rfft applied to c_k / N Y_k, overlap-add = adjoint of framing: the inverse ops run on
# the BACKWARD entry points of the analysis ops (and their gradients on the forward ones).
def _real_dtype(t):
    return {torch.complex64: torch.float32, torch.complex128: torch.float64}.get(t.dtype, t.dtype)


def _irfft_scale(yr, fft_length):
    """yr: (..., K, 2) real view of the half spectrum -> c_k / N * yr (ifftr.py:138)."""
    K = fft_length // 2 + 1
    out = torch.empty_like(yr)
    with torch.cuda.device(yr.device):
        _call("dsa_irfft_scale", _p(yr), yr.numel() // (2 * K), fft_length, _dtype_code(yr), _p(out), _stream())
    return out


def _div_rows(x2, d, eps=1e-16):
    out = torch.empty_like(x2)
    with torch.cuda.device(x2.device):
        _call("dsa_div_rows", _p(x2), x2.size(0), x2.size(1), _p(d), float(eps), _dtype_code(x2), _p(out), _stream())
    return out


def _fold_plan(N, L, P, center, out_length):
    """Signal length T the caller gets (unframe.py:176-192) and the length / frame count (Tc, Nc) the adjoint
    kernels are run with: Nc = num_frames(Tc) >= N (missing frames are zero), Tc >= T."""
    left = L // 2 if center else 0
    full = (N - 1) * P + L - left
    if out_length is None:
        T = N * P if center else full
    else:
        T = out_length
    T = max(0, min(T, full))        # slicing past the folded signal just ends there
    Tc = T if (T > 0 and num_frames(T, P) >= N) else max(T, (N - 1) * P + 1)
    return T, Tc, num_frames(Tc, P)


def _pad_frames(t, N, Nc, dim):
    if Nc == N:
        return t
    shape = list(t.shape)
    shape[dim] = Nc - N
    return torch.cat((t, t.new_zeros(shape)), dim=dim)


def _window_sq_sum(w, N, Nc, L, P, center, Tc):
    """Overlap-added squared window of the N frames, (Tc,): the divisor of unframe.py:204."""
    fr = (w * w).reshape(1, 1, L).expand(1, N, L)
    fr = _pad_frames(fr, N, Nc, 1).contiguous()
    d = torch.empty(1, Tc, device=w.device, dtype=w.dtype)
    with torch.cuda.device(w.device):
        _call("dsa_frame_bwd", _p(fr), 1, Tc, L, P, int(center), 0, 0, _dtype_code(fr), _p(d), _stream())
    return d.reshape(Tc)


class IfftrFn(torch.autograd.Function):
    """x:(..., out_length) = irfft(y:(..., L/2+1))[..., :out_length]  (ifftr.py:131-142)."""

    @staticmethod
    def forward(ctx, y, fft_length, out_length, twiddle):
        _require_device(y, twiddle)
        yr = torch.view_as_real(y.resolve_conj()).contiguous()
        _same_dtype(yr, twiddle)   # complex128 spectra need float64 tables: the kernels do not promote
        K = fft_length // 2 + 1
        F = yr.numel() // (2 * K)
        G = _irfft_scale(yr, fft_length)
        x0 = torch.zeros(F, out_length, device=y.device, dtype=yr.dtype)   # the adjoint is linear: any valid point
        x = torch.empty(*y.shape[:-1], out_length, device=y.device, dtype=yr.dtype)
        with torch.cuda.device(y.device):
            _call("dsa_fftr_bwd", _p(G), _p(x0), F, out_length, fft_length, 0, _p(twiddle), _dtype_code(yr), _p(x), _stream())
        ctx.save_for_backward(twiddle)
        ctx.cfg = (fft_length, out_length)
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, gx):
        (twiddle,) = ctx.saved_tensors
        fft_length, out_length = ctx.cfg
        gx = gx.contiguous()
        K = fft_length // 2 + 1
        F = gx.numel() // out_length
        Y = torch.empty(*gx.shape[:-1], K, 2, device=gx.device, dtype=gx.dtype)
        with torch.cuda.device(gx.device):
            _call("dsa_fftr_fwd", _p(gx), F, out_length, fft_length, 0, _p(twiddle), _dtype_code(gx), _p(Y), _stream())
        return torch.view_as_complex(_irfft_scale(Y, fft_length)), None, None, None


class UnframeFn(torch.autograd.Function):
    """x:(..., T) = overlap-add(y * w) / overlap-add(w^2)  (unframe.py:164-211); y:(..., N, L)."""

    @staticmethod
    def forward(ctx, y, w, P, center, out_length):
        _require_device(y, w)
        _same_dtype(y, w)
        if y.dim() <= 1:
            raise ValueError("Input must be at least 2D tensor.")
        yc, wc = y.contiguous(), w.contiguous()
        N, L = yc.shape[-2:]
        B = yc.numel() // (N * L)
        T, Tc, Nc = _fold_plan(N, L, P, center, out_length)
        yw = torch.empty_like(yc)
        num = torch.empty(B, Tc, device=y.device, dtype=y.dtype)
        with torch.cuda.device(y.device):
            _call("dsa_window_fwd", _p(yc), B * N, L, _p(wc), L, _dtype_code(yc), _p(yw), _stream())
            ywp = _pad_frames(yw.reshape(B, N, L), N, Nc, 1).contiguous()
            _call("dsa_frame_bwd", _p(ywp), B, Tc, L, P, int(center), 0, 0, _dtype_code(yc), _p(num), _stream())
        d = _window_sq_sum(wc, N, Nc, L, P, center, Tc)
        x = _div_rows(num, d)
        ctx.save_for_backward(wc, d)
        ctx.cfg = (yc.shape, P, center, T, Tc, Nc)
        return x[:, :T].reshape(*yc.shape[:-2], T)

    @staticmethod
    @once_differentiable
    def backward(ctx, gx):
        wc, d = ctx.saved_tensors
        shape, P, center, T, Tc, Nc = ctx.cfg
        N, L = shape[-2:]
        B = gx.numel() // max(T, 1)
        g2 = gx.reshape(B, T)
        if Tc != T:
            g2 = torch.cat((g2, g2.new_zeros(B, Tc - T)), dim=1)
        g2 = _div_rows(g2.contiguous(), d)
        fr = torch.empty(B, Nc, L, device=gx.device, dtype=gx.dtype)
        gy = torch.empty(B * N, L, device=gx.device, dtype=gx.dtype)
        with torch.cuda.device(gx.device):
            _call("dsa_frame_fwd", _p(g2), B, Tc, L, P, int(center), 0, 0, _dtype_code(g2), _p(fr), _stream())
            frn = fr[:, :N].contiguous()
            _call("dsa_window_fwd", _p(frn), B * N, L, _p(wc), L, _dtype_code(frn), _p(gy), _stream())
        return gy.reshape(shape), None, None, None, None


class IstftFn(torch.autograd.Function):
    """x:(..., T) = unframe(irfft(y)[..., :L])  (istft.py:186-193), fused: the complex-cotangent STFT backward
    kernel IS windowed inverse FFT + overlap-add."""

    @staticmethod
    def forward(ctx, y, window, twiddle, L, P, fft_length, center, out_length, algo):
        _require_device(y, window, twiddle)
        yr = torch.view_as_real(y.resolve_conj()).contiguous()
        _same_dtype(yr, window, twiddle)   # complex128 spectra need float64 tables: the kernels do not promote
        wc = window.contiguous()
        N, K = yr.shape[-3:-1]
        B = yr.numel() // (N * K * 2)
        T, Tc, Nc = _fold_plan(N, L, P, center, out_length)
        G = _pad_frames(yr.reshape(B, N, K, 2), N, Nc, 1).contiguous()
        d = _window_sq_sum(wc, N, Nc, L, P, center, Tc)
        x = torch.empty(B, Tc, device=y.device, dtype=yr.dtype)
        with torch.cuda.device(y.device):   # inverse weights while loading, overlap-add, division by d + 1e-16: one entry
            _call("dsa_istft_fwd", _p(G), B, Tc, L, P, fft_length, _p(wc), _p(twiddle), int(center), _p(d), 1e-16,
                  _dtype_code(yr), algo, _p(x), _stream())
        ctx.save_for_backward(wc, twiddle, d)
        ctx.cfg = (y.shape, L, P, fft_length, center, T, Tc, Nc, algo)
        return x[:, :T].reshape(*y.shape[:-2], T)

    @staticmethod
    @once_differentiable
    def backward(ctx, gx):
        wc, twiddle, d = ctx.saved_tensors
        shape, L, P, fft_length, center, T, Tc, Nc, algo = ctx.cfg
        N, K = shape[-2:]
        B = gx.numel() // max(T, 1)
        g2 = gx.reshape(B, T)
        if Tc != T:
            g2 = torch.cat((g2, g2.new_zeros(B, Tc - T)), dim=1)
        g2 = _div_rows(g2.contiguous(), d)
        Y = torch.empty(B, Nc, K, 2, device=gx.device, dtype=gx.dtype)
        with torch.cuda.device(gx.device):
            _call("dsa_stft_fwd", _p(g2), B, Tc, L, P, fft_length, _p(wc), _p(twiddle), int(center), 0, 0, 0.0, 0, 0.0, 5,
                  _dtype_code(g2), algo, _p(Y), _stream())   # format 5: complex output times c_k / nfft
        gy = Y[:, :N].contiguous()
        return (torch.view_as_complex(gy).reshape(shape),) + (None,) * 8


def griffin_update(t, y, phase, t_prev, d_prev, first, alpha, beta, gamma, eps, out=None):
    """One Griffin-Lim phase update (griffin.py:263-284, element-wise part): returns the next complex
    spectrogram sqrt(y + 1e-16) c / (|c| + eps); t_prev / d_prev (real views, (..., K, 2)) are updated in place.
    t=None is the initial step (phase=None: zeros)."""
    _require_device(y)
    _same_dtype(y, phase, t_prev, d_prev)
    K = y.size(-1)
    N = y.size(-2) if y.dim() >= 2 else 1
    B = y.numel() // max(N * K, 1)
    z = out if out is not None else torch.empty(*y.shape, dtype=torch.complex64 if y.dtype == torch.float32 else torch.complex128,
                                                device=y.device)
    zr = torch.view_as_real(z)
    tr, Nt = None, N
    if t is not None:
        if not t.is_complex() or t.size(-1) != K or t.size(-2) < N:
            raise ValueError("griffin_update: t must be the complex STFT of the current estimate")
        tr = torch.view_as_real(t.resolve_conj()).contiguous()
        Nt = t.size(-2)
    with torch.cuda.device(y.device):
        _call("dsa_griffin_update", _p(tr) if tr is not None else None, B, Nt, N, K, _p(y), _p(phase) if phase is not None else None,
              _p(t_prev), _p(d_prev), int(bool(first)), float(alpha), float(beta), float(gamma), float(eps), _dtype_code(y),
              _p(zr), _stream())
    return z
